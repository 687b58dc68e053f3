"""Register / scratch budgets of the kernels the ECVRF calls add (ed25519_VRF_Prove_*, ed25519_VRF_Verify_*,
ed25519_VRF_ProofToHash_*), from the compiler's own remarks (tools/resource_usage.kernel_usage: hipcc
-Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch -- x, k, the window tables and the points between the
walks live in registers, the tail words taken by value are read from the kernel arguments -- and no more registers (VGPR + AGPR) than
their launch bounds leave a lane: 256 at the two waves per SIMD of Prove and ProofToHash, 512 at Verify's one (it keeps two
projective window rows, the running point and the points already computed side by side).  The inversions run in the lane: the
calls launch no k_batch_invert, and no instance of it with a finisher of theirs exists."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

# launch bounds of csrc/engine_vrf.hip: 256 lanes a workgroup at 2, 1 and 2 waves per SIMD of 512 registers a lane
BUDGET = {"k_ed25519_vrf_prove": 256, "k_ed25519_vrf_verify": 512, "k_ed25519_vrf_proof_to_hash": 256}
OTHER_PREFIXES = ("k_h2c_", "k_ed25519_group_", "k_ed25519_key_", "k_ed25519_private_to_", "k_sc25519_")
OTHER_SUBSTRINGS = ("ristretto", "rist_", "zip215", "batcheq", "keyeq", "FinishGroup", "FinishKeyX25519", "FinishVerifyZip215",
                    "FinishVerifyIndexed", "FinishH2c", "FinishX25519,")


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0, k
    assert regs(k) <= BUDGET[name], k
    assert k.get("occupancy", 0) >= 512 // BUDGET[name], k


def test_no_other_kernel_was_added(usage):
    assert {n for n in usage if n.startswith("k_ed25519_vrf_")} == set(BUDGET)
    assert not [n for n in usage if "vrf" in n.lower() and n not in BUDGET], "the inversions are the lane's own"


def test_the_names_stay_out_of_the_other_features_patterns(usage):
    for n in BUDGET:
        assert not n.startswith(OTHER_PREFIXES), n
        assert not any(s in n for s in OTHER_SUBSTRINGS), n
