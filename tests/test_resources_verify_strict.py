"""Register / scratch budgets of the strict verification kernels against their plain twins, from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

TWINS = ["k_ed25519_verify_fast_scalars", "k_ed25519_verify_fast_points", "k_ed25519_verify_quad_prep", "k_ed25519_verify_quad_walk",
         "k_ed25519_verify_one_per_group"]


def waves(k):
    return min(8, 512 // (((regs(k) + 7) // 8) * 8))


@pytest.mark.parametrize("name", TWINS)
def test_strict_twin_is_spill_free_at_its_twins_occupancy(usage, name):
    plain, strict = usage[name], usage[name + "_strict"]
    assert strict.get("scratch", 0) == 0 and strict.get("vgpr_spill", 0) == 0, strict
    assert waves(strict) >= waves(plain), (strict, plain)
    assert strict.get("occupancy", 0) >= plain.get("occupancy", 0), (strict, plain)


def test_verify_check_strict_mask_is_spill_free(usage):
    k = usage["k_ed25519_verify_check_strict_mask"]
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0, k


def test_strict_lane_path_adds_no_walk_kernel(usage):
    """the strict lane path reuses k_ed25519_verify_fast_walk (a rejected element is marked as listed): no twin of the walk"""
    assert "k_ed25519_verify_fast_walk" in usage and "k_ed25519_verify_fast_walk_strict" not in usage
