"""Register / scratch budgets of the kernels the group calls add (ed25519_ScalarMult[_noclamp]_*, ed25519_ScalarMultBase[_noclamp]_*,
ed25519_PointAdd_*, ed25519_PointSub_*), from the compiler's own remarks (tools/resource_usage.kernel_usage: hipcc
-Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch, and no more registers (VGPR + AGPR) than the waves
per SIMD their launch bounds ask for leave a lane -- 512 / 2 for the variable-base walk at W = 2 and for the addition, 512 for the
walk at W = 3 and 4 and for the shared inversion's lone wave per SIMD, 512 / 4 for the walk over the wide comb."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

GROUPS = [16, 14, 12, 8, 4, 2, 1]          # launch_invert_k (engine_common.cuh): every group size is instantiated
BUDGET = {"k_ed25519_group_scalarmult<2>": 256, "k_ed25519_group_scalarmult<3>": 512, "k_ed25519_group_scalarmult<4>": 512,
          "k_ed25519_group_base": 128, "k_ed25519_group_add": 256}
BUDGET.update({f"k_batch_invert<c25519::FinishGroupPoint, {k}>": 512 for k in GROUPS})


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= BUDGET[name], k


def test_no_other_kernel_was_added(usage):
    mine = {n for n in usage if "FinishGroup" in n or n.startswith("k_ed25519_group_")}
    assert mine == set(BUDGET), sorted(mine ^ set(BUDGET))
