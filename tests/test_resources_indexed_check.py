"""Register / scratch budgets of the kernels behind ed25519_Verify_Check_indexed_* (many contexts in one call), from the compiler's
own remarks (tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950)."""
from kernel_usage import regs, usage  # noqa: F401


def test_per_lane_kernel_fits_two_waves_per_simd(usage):
    """k_ed25519_verify_check_indexed: __launch_bounds__(ED_BLOCK, 2) like k_ed25519_verify_check_shared -- at most 168 registers
    and no scratch"""
    k = usage["k_ed25519_verify_check_indexed"]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= 168, k


def test_per_wave_kernel_within_its_bound(usage):
    """k_ed25519_verify_check_indexed_coop: one wave per pair, amdgpu_waves_per_eu(1, 4) like k_ed25519_verify_check_coop (128
    registers), no scratch"""
    k = usage["k_ed25519_verify_check_indexed_coop"]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= 128, k
    assert regs(k) <= regs(usage["k_ed25519_verify_check_coop"]) + 8, k


def test_index_aware_inversion_is_instantiated_spill_free(usage):
    """k_batch_invert<FinishVerifyIndexed, K> for every group size the launch can pick"""
    inv = {n: k for n, k in usage.items() if n.startswith("k_batch_invert<c25519::FinishVerifyIndexed")}
    assert len(inv) == 7, sorted(inv)
    for n, k in inv.items():
        assert k.get("scratch", 0) == 0, (n, k)
