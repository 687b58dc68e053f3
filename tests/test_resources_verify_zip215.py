"""Register / scratch budgets of the ZIP-215 verification kernels against their plain twins, from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

TWINS = ["k_ed25519_verify_fast_scalars", "k_ed25519_verify_fast_points", "k_ed25519_verify_quad_prep", "k_ed25519_verify_quad_walk",
         "k_ed25519_verify_one_per_group", "k_ed25519_verify_slow"]


def waves(k):
    return min(8, 512 // (((regs(k) + 7) // 8) * 8))


@pytest.mark.parametrize("name", TWINS)
def test_zip215_twin_is_spill_free_at_its_twins_occupancy(usage, name):
    plain, twin = usage[name], usage[name + "_zip215"]
    assert twin.get("scratch", 0) == 0 and twin.get("vgpr_spill", 0) == 0, twin
    assert waves(twin) >= waves(plain), (twin, plain)
    assert twin.get("occupancy", 0) >= plain.get("occupancy", 0), (twin, plain)


def test_every_shape_has_its_zip215_kernels_and_the_lane_path_no_walk_of_its_own(usage):
    """six new kernels: the three shapes of the lattice path and the cofactored reference-order kernel behind them.  The lane path
    reuses k_ed25519_verify_fast_walk on scalars multiplied by 8 (a twin of that kernel changes its gfx950 code): no walk twin"""
    assert sorted(k for k in usage if "zip215" in k) == sorted(n + "_zip215" for n in TWINS)
    assert "k_ed25519_verify_fast_walk" in usage and "k_ed25519_verify_fast_walk_zip215" not in usage
