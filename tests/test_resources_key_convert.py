"""Register / scratch budgets of the kernels the key calls add (ed25519_ClassifyKey_*, ed25519_PublicKey_to_X25519_*,
ed25519_PrivateKey_to_X25519_*), from the compiler's own remarks (tools/resource_usage.kernel_usage: hipcc
-Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): no scratch, and no more registers (VGPR + AGPR) than the waves
per SIMD their launch bounds ask for leave a lane -- 512 / 2 for the two walk kernels, 512 for a 256-lane workgroup without an
occupancy target and for the shared inversion's lone wave per SIMD."""
import pytest

from kernel_usage import regs, usage  # noqa: F401

GROUPS = [16, 14, 12, 8, 4, 2, 1]          # launch_invert_k (engine_common.cuh): every group size is instantiated
BUDGET = {"k_ed25519_key_classify": 256, "k_ed25519_key_to_x25519": 256, "k_ed25519_private_to_x25519": 512}
BUDGET.update({f"k_batch_invert<c25519::FinishKeyX25519, {k}>": 512 for k in GROUPS})


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_new_kernel_has_no_scratch_and_fits_its_launch_bounds(usage, name):
    k = usage[name]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= BUDGET[name], k


def test_no_other_kernel_was_added(usage):
    mine = {n for n in usage if "FinishKeyX25519" in n or n.startswith(("k_ed25519_key_", "k_ed25519_private_to_"))}
    assert mine == set(BUDGET), sorted(mine ^ set(BUDGET))
