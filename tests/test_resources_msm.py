"""Register / scratch budgets of the kernels the multiscalar calls add (csrc/engine_msm.hip), from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch memory and no
spill, and no more registers (VGPR + AGPR) than their launch bounds leave a lane -- 256 at the two waves per SIMD of the rows, the
sum, the finish and the bucket path's point rows (template argument 0: edwards25519, 1: ristretto255), 512 for the unconstrained workgroups of the clear, the
scalars and the tail.  The bucket path's count / scan / scatter / buckets / windows stages are the batch equation's kernels
(tests/test_resources_verify_batch.py, tests/test_resources_verify_batch_indexed.py) and add none."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

BUDGET = {"k_msm_rows<0>": 256, "k_msm_rows<1>": 256, "k_msm_sum": 256, "k_msm_finish<0>": 256, "k_msm_finish<1>": 256,
          "k_msm_points<0>": 256, "k_msm_points<1>": 256, "k_msm_clear": 512, "k_msm_scalars": 512, "k_msm_tail<0>": 512, "k_msm_tail<1>": 512}
OTHER_SUBSTRINGS = ("batcheq", "keyeq", "zip215", "ristretto", "rist_", "k_ed25519_group_", "vrf", "oprf", "FinishGroup")


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_no_spill_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
    assert regs(k) <= BUDGET[name], k
    assert k.get("occupancy", 0) >= 512 // BUDGET[name], k


def test_the_set_of_kernels_is_exactly_the_listed_one(usage):
    assert {n for n in usage if "k_msm_" in n} == set(BUDGET)


def test_the_names_stay_out_of_the_other_features_patterns():
    for n in BUDGET:
        assert not any(s.lower() in n.lower() for s in OTHER_SUBSTRINGS), n
