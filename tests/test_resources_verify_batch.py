"""Register / scratch budgets of the ZIP-215 batch equation's kernels (csrc/engine_batch_eq.hip), from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
import pytest

from kernel_usage import usage  # noqa: F401

KERNELS = ["points", "scalars", "count", "scan", "scatter", "buckets", "windows", "tail", "and"]


def test_the_equation_has_its_kernels_and_none_is_a_zip215_twin(usage):
    """tests/test_resources_verify_zip215.py asserts the exact set of kernels whose name contains zip215: these must stay out of it"""
    mine = sorted(k for k in usage if "batcheq" in k)
    assert mine == sorted("k_ed25519_batcheq_" + n for n in KERNELS)
    assert not any("zip215" in k for k in mine)


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_is_spill_free(usage, name):
    k = usage["k_ed25519_batcheq_" + name]
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k


def test_the_per_point_and_per_bucket_kernels_keep_four_waves_per_simd(usage):
    """decoding (one square root per lane) and the bucket sums are the stages every point passes through: 128 registers or fewer"""
    for name in ("points", "scalars", "buckets"):
        k = usage["k_ed25519_batcheq_" + name]
        assert k["vgpr"] + k.get("agpr", 0) <= 128, k
