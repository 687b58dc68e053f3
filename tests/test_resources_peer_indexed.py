"""Register / scratch budgets of the kernels behind curve25519_dh_Peer_Init_* and curve25519_dh_CreateSharedKey_indexed_* (many peer
contexts in one call), from the compiler's own remarks (tools/resource_usage.kernel_usage: hipcc -Rpass-analysis=kernel-resource-usage,
cross-compiled for gfx950)."""
from kernel_usage import regs, usage  # noqa: F401


def test_walk_fits_four_waves_per_simd(usage):
    """k_x25519_peer_indexed_walk: __launch_bounds__(WB_BLOCK, 4) like k_x25519_one_peer_mult -- at most 128 registers, no scratch"""
    k = usage["k_x25519_peer_indexed_walk"]
    assert k.get("scratch", 0) == 0, k
    assert regs(k) <= 128, k


def test_ladder_and_gather_kernels_spill_free(usage):
    """the ladder over the listed elements within k_x25519_ladder's budget; the context build and the key gather without scratch"""
    lad = usage["k_x25519_peer_indexed_ladder"]
    assert lad.get("scratch", 0) == 0 and regs(lad) <= 128, lad
    for name in ("k_x25519_peer_init", "k_x25519_peer_gather"):
        assert usage[name].get("scratch", 0) == 0, usage[name]
    assert regs(usage["k_x25519_peer_init"]) <= 256, usage["k_x25519_peer_init"]


def test_inversion_instantiations_spill_free(usage):
    """k_batch_invert<FinishX25519, K>, which the indexed call shares with the ladder's split path, for every group size"""
    inv = {n: k for n, k in usage.items() if n.startswith("k_batch_invert<FinishX25519,")}
    assert len(inv) == 7, sorted(inv)
    for n, k in inv.items():
        assert k.get("scratch", 0) == 0, (n, k)
