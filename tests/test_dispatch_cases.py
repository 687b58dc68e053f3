"""CPU suite: the case sets of tests/dispatch_cases.py are what tests/test_gpu_dispatch_edges.py's assertions rest on -- checked
with the oracle alone, before any of them reaches a device.  These are conditions on the inputs, not measurements of the library."""
import numpy as np
import pytest

import dispatch_cases as dc
from vectors import P, ed_decode


def test_sizes_sit_on_both_sides_of_every_threshold():
    for sizes, thresholds in ((dc.X25519_SIZES, (512, 3584, 1 << 15, 1 << 16)), (dc.FIXED_BASE_SIZES, (1024, 1 << 14)),
                              (dc.VERIFY_SIZES, (1024, 1 << 15)), (dc.BLINDED_SIZES, (2048,))):
        for t in thresholds:
            assert t in sizes and t + 1 in sizes, (sizes, t)
    for lengths, sizes in ((dc.FIXED_BASE_LENGTHS, dc.FIXED_BASE_SIZES), (dc.VERIFY_LENGTHS, dc.VERIFY_SIZES),
                           (dc.BLINDED_LENGTHS, dc.BLINDED_SIZES)):
        assert tuple(sorted(lengths)) == sizes
        assert set().union(*lengths.values()) == set(dc.MSG_LENGTHS)
        assert set(lengths[max(n for n in sizes if n <= 32769)]) == set(dc.MSG_LENGTHS)      # the open-ended form: all six at its first size
    assert set(dc.FIRST_LENGTHS) | set(dc.LAST_LENGTHS) == set(dc.MSG_LENGTHS)
    for first in (1025,):
        assert dc.FIXED_BASE_LENGTHS[first] == dc.VERIFY_LENGTHS[first] == dc.FIRST_LENGTHS
    for last in (1024, 16384):
        assert dc.FIXED_BASE_LENGTHS[last] == dc.LAST_LENGTHS
    for last in (1024, 32768):
        assert dc.VERIFY_LENGTHS[last] == dc.LAST_LENGTHS


def test_edge_rows_reach_the_ragged_tail():
    for n in (513, 3585, 32769, 65537):
        assert (n - 1) & ~63 == n - 1 and dc.edge_rows(n) == [n - 1, n - 2, 0]          # the last wave holds row n - 1 alone
    assert dc.edge_rows(512) == [511, 510, 448, 0] and dc.edge_rows(2) == [1, 0]
    last = [dc.last_row_peer(n) for n in dc.X25519_SIZES]
    assert any(v % P in dc.LOW_ORDER_U for v in last), "the last row is a low-order point at some sizes ..."
    assert any(v >= P for v in last), "... and a non-canonical encoding at others"
    lone = [dc.last_row_peer(n) % P in dc.LOW_ORDER_U for n in (513, 3585, 32769)]
    assert any(lone), "a wave whose only row has Z = 0"


@pytest.mark.parametrize("n", dc.X25519_SIZES)
def test_x25519_sets_hold_the_zero_rows_they_claim(oracle, n):
    pk, sk, low = dc.x25519_rows(n)
    assert pk.shape == sk.shape == (n, 32) and 1 <= low <= 4
    shared, clamped = oracle.x25519_shared(pk, sk, threads=dc.THREADS)
    zero = ~shared.any(axis=1)
    assert int(zero.sum()) == low
    assert set(np.nonzero(zero)[0]) <= set(dc.edge_rows(n))
    rows = dc.edge_rows(n)
    assert {bytes(sk[r]) for r in rows} == {bytes(32), b"\xff" * 32}                    # all-zero and all-ones secrets beside them
    assert (clamped[rows, 0] & 7 == 0).all() and (clamped[rows, 31] & 0xC0 == 0x40).all()


@pytest.mark.parametrize("n", dc.VERIFY_SIZES)
def test_verification_sets_mix_verdicts_in_their_last_rows(oracle, n):
    for mlen in dc.VERIFY_LENGTHS[n]:
        sig, pk, msg, bad_row = dc.verify_rows(oracle, n, mlen)
        assert sig.shape == (n, 64) and pk.shape == (n, 32) and msg.shape == (n, mlen)
        ok = oracle.ed25519_verify(sig, pk, msg, threads=dc.THREADS)
        tail = ok[n - dc.TAIL:]
        assert tail.any() and not tail.all(), (mlen, tail)
        assert n - dc.TAIL <= bad_row < n and ok[bad_row] == 0
        v = int.from_bytes(pk[bad_row].tobytes(), "little")
        assert (v & dc.MASK255) < P and ed_decode(v & dc.MASK255, v >> 255) is None
        share = ok.mean()
        assert 0.25 <= share <= 0.75, (mlen, share)
        assert ok[1] == 1 and ok[0] == 0 and ok[2] == 0 and ok[4] == 0                      # an honest row, and a flip of each kind


def test_rebuilt_edges_have_their_length_and_both_verdicts(oracle):
    seen = set()
    for mlen in dc.MSG_LENGTHS:
        edges = dc.rebuilt_edges(mlen)
        assert len(edges) == 4 and all(len(s) == 64 and len(a) == 32 and len(m) == mlen for s, a, m in edges)
        f = lambda k: np.stack([np.frombuffer(e[k], np.uint8) for e in edges])  # noqa: E731
        ok = oracle.ed25519_verify(f(0), f(1), f(2))
        assert ok[0] == 1, "the mixed-order key's signature satisfies the cofactorless equation"
        seen |= set(ok.tolist())
    assert seen == {0, 1}
