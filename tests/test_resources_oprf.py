"""Register / scratch budgets of the kernels the OPRF / VOPRF calls add, from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch memory and no
spill, and no more registers (VGPR + AGPR) than their launch bounds leave a lane -- 256 at the two waves per SIMD of the per-row
kernels and of both row stages (the server's builds C_i's table twice rather than keep it under the encoding of D_i; the verifier's
runs a lane per point), 512 at the one wave of the per-request stages and of the one-lane head kernels."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

BUDGET = {"k_oprf_blind": 256, "k_oprf_finalize": 256, "k_oprf_evaluate": 256, "k_oprf_server_rows": 256, "k_oprf_verifier_rows": 256,
          "k_oprf_server_head": 512, "k_oprf_verifier_head": 512, "k_oprf_prove": 512, "k_oprf_check": 512}
OTHER_PREFIXES = ("k_h2c_", "k_ed25519_group_", "k_ed25519_key_", "k_ed25519_private_to_", "k_sc25519_", "k_ed25519_vrf_", "k_batch_invert")
OTHER_SUBSTRINGS = ("ristretto", "rist_", "vrf", "zip215", "batcheq", "keyeq", "FinishGroup", "FinishKeyX25519", "FinishVerifyZip215",
                    "FinishVerifyIndexed", "FinishH2c", "FinishX25519,", "verify_check")


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0, k
    assert regs(k) <= BUDGET[name], k
    assert k.get("occupancy", 0) >= 512 // BUDGET[name], k


def test_no_other_kernel_was_added(usage):
    assert {n for n in usage if n.startswith("k_oprf_")} == set(BUDGET)
    assert not [n for n in usage if "oprf" in n.lower() and n not in BUDGET], "the inversions are the lane's own"


def test_the_names_stay_out_of_the_other_features_patterns(usage):
    for n in BUDGET:
        assert not n.startswith(OTHER_PREFIXES), n
        assert not any(s in n.lower() for s in (s.lower() for s in OTHER_SUBSTRINGS)), n
