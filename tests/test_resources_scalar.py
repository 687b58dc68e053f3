"""Register / scratch budgets of the kernels the scalar calls add (ed25519_ScalarReduce_*, _ScalarAdd_*, _ScalarSub_*, _ScalarMul_*,
_ScalarNegate_*, _ScalarComplement_*, _ScalarMulAdd_*, _ScalarInvert_*, _ScalarIsCanonical_*), from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch, and no more
registers (VGPR + AGPR) than the two waves per SIMD their launch bounds ask for leave a lane, 512 / 2 -- the inversion at K = 16
included, whose prefix products are what fills them.  The calls lease no scratch: these seven kernels are all they run."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

BUDGET = {"k_sc25519_op": 256, "k_sc25519_is_canonical": 256, "k_sc25519_invert<1>": 256, "k_sc25519_invert<2>": 256,
          "k_sc25519_invert<4>": 256, "k_sc25519_invert<8>": 256, "k_sc25519_invert<16>": 256}
LDS_PER_CU = 160 * 1024


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= BUDGET[name], k
    assert 2 * k.get("lds", 0) <= LDS_PER_CU, "two workgroups of 256 lanes per CU are the two waves per SIMD"


def test_no_other_kernel_was_added(usage):
    mine = {n for n in usage if n.startswith("k_sc25519_")}
    assert mine == set(BUDGET), sorted(mine ^ set(BUDGET))
