"""Register / scratch budgets of the kernels behind ed25519_Sign_Init_* and ed25519_SignMessage_indexed_* (many signer contexts in one
call), from the compiler's own remarks (tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage,
cross-compiled for gfx950).  Each indexed kernel is held to the occupancy its launch bounds ask for and to the registers of the
ed25519_SignMessage kernel it mirrors."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

# new kernel -> (register budget of its launch bounds, the ed25519_SignMessage kernel it mirrors)
KERNELS = {
    "k_ed25519_sign_indexed_mult<true>": (128, "k_ed25519_sign_mult<false, true>"),        # __launch_bounds__(WB_BLOCK, 4)
    "k_ed25519_sign_indexed_mult<false>": (128, "k_ed25519_sign_mult<false, false>"),      # __launch_bounds__(BM_BLOCK, 4)
    "k_ed25519_sign_indexed_finish": (128, "k_ed25519_sign_finish"),                       # the budget test_resources.py gives it
    "k_ed25519_sign_indexed_quad": (256, "k_ed25519_sign_quad"),                           # amdgpu_waves_per_eu(1, 2)
    "k_ed25519_sign_indexed_coop<true>": (168, "k_ed25519_sign_coop<true>"),               # two waves per workgroup, three per SIMD
    "k_ed25519_sign_indexed_coop<false>": (168, "k_ed25519_sign_coop<false>"),
}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_indexed_kernel_spill_free_within_its_bounds(usage, name):
    """no scratch, registers within the launch bounds' occupancy, and no more than the single-key kernel's (+ 8), so the indexed
    call runs as many waves per SIMD as ed25519_SignMessage_dev does"""
    budget, twin = KERNELS[name]
    k = usage[name]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= budget, k
    assert regs(k) <= regs(usage[twin]) + 8, (k, usage[twin])
    assert k["occupancy"] >= usage[twin]["occupancy"], (k, usage[twin])


def test_context_build_spill_free(usage):
    """k_ed25519_sign_ctx_init: one lane per key, no scratch"""
    k = usage["k_ed25519_sign_ctx_init"]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= 128, k
