"""Register / scratch budgets of the kernels ed25519_Verify_Check_zip215_* adds, from the compiler's own remarks
(tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage, cross-compiled for gfx950): every one spill-free."""
import pytest

from kernel_usage import spill_free, usage  # noqa: F401

PLAIN = ["k_ed25519_verify_coset_prep", "k_ed25519_verify_coset_key_gather", "k_ed25519_verify_coset_index_mask"]
GROUPS = [12, 8, 4, 2, 1]          # launch_coset_finish (engine_verify_ctx.hip): this finish is instantiated up to 12 elements per lane


@pytest.mark.parametrize("name", PLAIN)
def test_new_kernel_is_spill_free(usage, name):
    assert spill_free(usage[name]), usage[name]


@pytest.mark.parametrize("k", GROUPS)
def test_coset_finish_is_spill_free(usage, k):
    name = f"k_batch_invert<c25519::FinishVerifyZip215, {k}>"
    assert spill_free(usage[name]), usage[name]


def test_no_other_group_size_and_no_twin_of_a_walk(usage):
    """the sizes that spilled (14, 16) are not instantiated, and the context walks have no ZIP-215 twin: the plain kernels are launched"""
    mine = sorted(n for n in usage if "FinishVerifyZip215" in n)
    assert mine == sorted(f"k_batch_invert<c25519::FinishVerifyZip215, {k}>" for k in GROUPS), mine
    for walk in ("k_ed25519_verify_check_indexed", "k_ed25519_verify_check_shared", "k_ed25519_verify_check_wide"):
        assert walk in usage and not any(n.startswith(walk) and "zip215" in n for n in usage)
    assert {n for n in usage if "zip215" in n and "verify_check" in n} == set()
