"""Register / scratch budgets of the kernels the hashing calls add (c25519_ExpandMessageXmd_*, ed25519_MapToCurve_*,
ed25519_HashToCurve_*, ed25519_EncodeToCurve_*, ristretto255_HashToGroup_*, ed25519_HashToScalar_*), from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch -- the tail
words taken by value are read from the kernel arguments, not copied to a lane's stack -- and no more registers (VGPR + AGPR) than the
two waves per SIMD of their launch bounds leave a lane.  The Edwards encoding's inversion runs in the lane: the calls launch no
k_batch_invert, and no instance of it with a finisher of theirs exists."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

BUDGET = {"k_h2c_expand": 256, "k_h2c_map": 256, "k_h2c_to_curve<1>": 256, "k_h2c_to_curve<2>": 256, "k_h2c_to_group": 256,
          "k_h2c_to_scalar": 256}


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= BUDGET[name], k


def test_no_other_kernel_was_added(usage):
    assert {n for n in usage if n.startswith("k_h2c_")} == set(BUDGET)
    assert not [n for n in usage if "FinishH2c" in n], "the inversion is the lane's own"


def test_the_names_stay_out_of_the_other_features_patterns(usage):
    for n in BUDGET:
        low = n.lower()
        assert "ristretto" not in low and "rist_" not in low
        assert not any(s in n for s in ("FinishGroup", "FinishKeyX25519", "FinishVerifyZip215", "FinishVerifyIndexed"))
        assert not n.startswith(("k_ed25519_group_", "k_ed25519_key_", "k_ed25519_private_to_", "k_sc25519_"))
