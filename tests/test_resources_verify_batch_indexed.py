"""Register / scratch budgets of the coalesced ZIP-215 batch equation's own kernels (k_ed25519_keyeq_* in csrc/engine_batch_eq.hip; the
scan, the buckets, the windows and the tail are the plain equation's: tests/test_resources_verify_batch.py), from the compiler's own
remarks (tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
import pytest

from kernel_usage import usage  # noqa: F401

KERNELS = ["points", "scalars", "fold", "count", "scatter", "gather"]


def test_the_coalesced_equation_has_its_kernels_under_their_own_name(usage):
    """tests/test_resources_verify_batch.py and test_resources_verify_zip215.py assert the exact sets of kernels whose names contain
    batcheq and zip215: these must stay out of both"""
    mine = sorted(k for k in usage if "keyeq" in k)
    assert mine == sorted("k_ed25519_keyeq_" + n for n in KERNELS)
    assert not any("zip215" in k or "batcheq" in k for k in mine)


@pytest.mark.parametrize("name", KERNELS)
def test_kernel_is_spill_free(usage, name):
    k = usage["k_ed25519_keyeq_" + name]
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k


def test_the_per_point_and_per_element_kernels_keep_four_waves_per_simd(usage):
    """decoding (one square root per lane), the scalars (two hashes and the per-key sums) and the fold: 128 registers or fewer"""
    for name in ("points", "scalars", "fold"):
        k = usage["k_ed25519_keyeq_" + name]
        assert k["vgpr"] + k.get("agpr", 0) <= 128, k


def test_the_scalars_kernel_keeps_four_workgroups_per_cu_in_lds(usage):
    """its table of per-key sums is 2 x 256 slots of a key and eight 64-bit words: four workgroups of it fit the CU's 160 KiB"""
    assert usage["k_ed25519_keyeq_scalars"]["lds"] * 4 <= 160 * 1024
