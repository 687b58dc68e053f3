"""Register / scratch budgets of the kernels the ristretto255 calls add (ristretto255_IsValidPoint_*, ristretto255_FromHash_*,
ristretto255_ScalarMult_*, ristretto255_ScalarMultBase_*, ristretto255_PointAdd_*, ristretto255_PointSub_*), from the compiler's own
remarks (tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch, and
no more registers (VGPR + AGPR) than the waves per SIMD their launch bounds ask for leave a lane -- 512 / 2 for decode -> walk ->
encode at W = 2 and for every kernel that is square-root chains alone, the comb's included; 512 for the walk at W = 3 and 4.  The
calls lease no scratch and launch no shared inversion: these seven kernels are all they run."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

BUDGET = {"k_ristretto255_scalarmult<2>": 256, "k_ristretto255_scalarmult<3>": 512, "k_ristretto255_scalarmult<4>": 512,
          "k_ristretto255_base": 256, "k_ristretto255_add": 256, "k_ristretto255_is_valid": 256, "k_ristretto255_from_hash": 256}


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= BUDGET[name], k


def test_no_other_kernel_was_added(usage):
    mine = {n for n in usage if "ristretto" in n.lower() or "rist_" in n.lower()}
    assert mine == set(BUDGET), sorted(mine ^ set(BUDGET))
