"""Register / scratch budgets of the ZIP-215 verification kernels against their plain twins, from the compiler's own remarks
(tools/resource_usage.compile_remarks: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TWINS = ["k_ed25519_verify_fast_scalars", "k_ed25519_verify_fast_points", "k_ed25519_verify_quad_prep", "k_ed25519_verify_quad_walk",
         "k_ed25519_verify_one_per_group", "k_ed25519_verify_slow"]


@pytest.fixture(scope="module")
def usage():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import resource_usage
    return {k["pretty"]: k for k in resource_usage.compile_remarks()}


def regs(k):
    return k["vgpr"] + k.get("agpr", 0)


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
