"""Inputs for the base calls at the sizes where their default dispatch changes form (tests/test_gpu_dispatch_edges.py runs them on
the device, tests/test_dispatch_cases.py checks with the oracle alone that they are what that test's assertions rest on).  No GPU
in here: seeds come from synth.random_bytes, expectations from the oracle.

A form's FIRST size is where its grid is smallest and its last wave, quad or workgroup most ragged (T + 1 for a threshold T); its
LAST size is where the grid is largest.  The edge rows sit where a ragged tail goes wrong: the last row, the one before it, the first
row of the last wave, row 0."""
import functools
import os

import numpy as np

from curve25519_amd import synth
from vectors import L, P, ED_B, ed_add, ed_decode, ed_enc, ed_mul, ed_order8_point, small_order_encodings

THREADS = min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS") or 0) or 1 << 30)   # as tests/test_gpu_parity.py: a share of a big host

MASK255 = 2**255 - 1

# ---- sizes: both sides of every default threshold ---------------------------------------------------------------------------
X25519_SIZES = (512, 513, 3584, 3585, 32768, 32769, 65536, 65537)
PUBLIC_KEY_SIZES = tuple(n for n in X25519_SIZES if n <= 32769)
FIXED_BASE_SIZES = (1024, 1025, 16384, 16385)
BLINDED_SIZES = (2, 65, 2048, 2049, 65537, 131073)
VERIFY_SIZES = (1024, 1025, 32768, 32769)
BATCH_SIZE = 32769                       # the *_batch forms: one call of each operation
ORACLE_MAX_BLINDED = 16385               # up to here the blinded calls are compared with the oracle too, not only with the unblinded call

# ---- message lengths: the last one-, two- and three-block message of H(enc(R) || pk || m) is 47, 175 bytes (48, 176 open the next
# block); of H(prefix || m) 79, 207 (80 opens the next) -------------------------------------------------------------------------
MSG_LENGTHS = (47, 48, 79, 80, 175, 176)
FIRST_LENGTHS = (47, 80, 175)            # the first size of a form's range
LAST_LENGTHS = (48, 79, 176)             # the last size


def _lengths(first_sizes, last_sizes, open_ended):
    out = {n: FIRST_LENGTHS for n in first_sizes}
    out.update({n: LAST_LENGTHS for n in last_sizes})
    out.update({n: MSG_LENGTHS for n in open_ended})       # a form with no upper end in the tested range: all six at its first size
    return out


FIXED_BASE_LENGTHS = _lengths(first_sizes=(1025,), last_sizes=(1024, 16384), open_ended=(16385,))
VERIFY_LENGTHS = _lengths(first_sizes=(1025,), last_sizes=(1024, 32768), open_ended=(32769,))
# the blinded calls have two forms: per wave up to 2048, one lane from 2049 on.  The two large sizes take one length from each side of
# a block edge (their cost is the host's copies, not the kernels)
BLINDED_LENGTHS = {2: FIRST_LENGTHS, 65: LAST_LENGTHS, 2048: LAST_LENGTHS, 2049: MSG_LENGTHS, 65537: (47, 176), 131073: (48, 175)}


def _le(v, nbytes=32):
    return np.frombuffer(int(v).to_bytes(nbytes, "little"), np.uint8)


# ---- X25519 ----------------------------------------------------------------------------------------------------------------
# 0 and 1 are low-order points (Z = 0 inside a shared inversion), p - 1 is the point of order 4 with u = -1, p is 0 again in a
# non-canonical encoding, 2^255 - 1 = p + 18, and 2^256 - 1 has bit 255 set, which the reference does not mask (= 37 mod p)
EDGE_PEERS = (0, 1, P - 1, P, 2**255 - 1, 2**256 - 1)
LOW_ORDER_U = (0, 1, P - 1)


def edge_rows(n):
    """the rows that get an edge input, from n - 1 downwards: n - 1, n - 2, the first row of the last wave, row 0 (each once)"""
    rows = []
    for r in (n - 1, n - 2, (n - 1) & ~63, 0):
        if 0 <= r < n and r not in rows:
            rows.append(r)
    return rows


def x25519_rows(n):
    """(pk[n, 32], sk[n, 32], low): seeded rows with the edge peer keys at edge_rows(n), placed in a rotation that starts at another
    key for another n (so the last row is a low-order point at some sizes and a non-canonical one at others), secrets of all-zero /
    all-ones bytes beside them.  low: how many of the placed keys are low-order points -- their shared key is 32 zero bytes."""
    pk = synth.random_bytes((n, 32), 0xD15A0000 + n)
    sk = synth.random_bytes((n, 32), 0xD15B0000 + n)
    low = 0
    for slot, r in enumerate(edge_rows(n)):
        v = EDGE_PEERS[(n // 3 + slot) % len(EDGE_PEERS)]
        pk[r] = _le(v)
        sk[r] = 0x00 if slot % 2 == 0 else 0xFF
        low += v % P in LOW_ORDER_U
    return pk, sk, low


def last_row_peer(n):
    return EDGE_PEERS[(n // 3) % len(EDGE_PEERS)]


# ---- key pairs and signatures ----------------------------------------------------------------------------------------------
def sign_rows(n, mlen):
    """(sk[n, 32], msg[n, mlen]): seeded; the secrets depend on n alone, so one key pair serves every length of a size"""
    return synth.random_bytes((n, 32), 0xD15C0000 + n), synth.random_bytes((n, mlen), 0xD15D0000 + 0x1000 * mlen + n % 0x1000)


# ---- verification ----------------------------------------------------------------------------------------------------------
def undecodable_key(seed):
    """a canonical 32-byte string (y < p) that is no point of the curve: the first such row of a seeded block, by vectors.ed_decode"""
    for row in synth.random_bytes((64, 32), seed):
        v = int.from_bytes(row.tobytes(), "little")
        if (v & MASK255) < P and ed_decode(v & MASK255, v >> 255) is None:
            return row.copy()
    raise AssertionError("no undecodable key in 64 seeded rows")


def _flip_r(sig, i):
    sig[i, i % 32] ^= np.uint8(1 << (i % 8))


def _flip_s(sig, i):
    sig[i, 32 + i % 31] ^= np.uint8(1 << (i % 8))          # (bytes 32..62: the top bits of S stay, so it is another residue mod L)


def _flip_m(msg, i):
    msg[i, -1] ^= np.uint8(0x80 >> (i % 8))


def _s_plus_l(sig, i):
    S = int.from_bytes(sig[i, 32:].tobytes(), "little") + L
    assert S < 2**256
    sig[i, 32:] = _le(S)


@functools.lru_cache(maxsize=None)
def rebuilt_edges(mlen):
    """[(sig, pk, msg)] as bytes: tests/strict_cases.py's edge_cases are 32-byte messages, so their kinds that depend on the hash
    are made again under an mlen-byte message (as zip215_cases.edge_set re-keys its own): a mixed-order key a*B + t*T8 with a
    signature whose cofactorless equation holds, the same with S + L, a small-order key with a small-order R and S = 0, and the first
    signature under a small-order key in a non-canonical encoding (y >= p).  The oracle decides the verdicts."""
    import random
    import strict_cases as sc
    rnd = random.Random(0xD15E00 + mlen)
    T8 = ed_order8_point()
    out = []
    a, t = rnd.getrandbits(252) % L, 1 + mlen % 7
    A = ed_enc(ed_add(ed_mul(a, ED_B), ed_mul(t, T8)))
    m = bytes(rnd.getrandbits(8) for _ in range(mlen))
    Rb, S = sc._sign_with(a, t, A, m, rnd)
    out.append((Rb + S.to_bytes(32, "little"), A, m))
    out.append((Rb + (S + L).to_bytes(32, "little"), A, m))
    encs = [e for e, _ in small_order_encodings()]
    out.append((encs[mlen % len(encs)] + bytes(32), encs[(3 * mlen + 1) % len(encs)], bytes([mlen & 0xFF]) * mlen))
    big = [e for e in encs if (int.from_bytes(e, "little") & MASK255) >= P]
    out.append((Rb + S.to_bytes(32, "little"), big[mlen % len(big)], m))
    return out


TAIL = 8                                 # the last rows of a verification set, which carry one input of every kind


@functools.lru_cache(maxsize=4)
def _keys(oracle, n):
    sk = synth.random_bytes((n, 32), 0xD15F0000 + n)
    return oracle.ed25519_keypair(sk, threads=THREADS)


def verify_rows(oracle, n, mlen):
    """(sig[n, 64], pk[n, 32], msg[n, mlen], bad_key_row): the ORACLE's signatures (not the code under test's); a bit flipped in R
    at rows 7k, in S at 7k + 2, in the last message byte at 7k + 4; and in the last TAIL rows, at places that rotate with n: one
    untouched signature, one flip of each kind, S + L, a key that does not decode, and two of rebuilt_edges(mlen)."""
    assert n >= 2 * TAIL
    pub, priv = _keys(oracle, n)
    msg = synth.random_bytes((n, mlen), 0xD1600000 + 0x1000 * mlen + n % 0x1000)
    sig = oracle.ed25519_sign(priv, msg, threads=THREADS)
    pk = pub.copy()
    body = np.arange(n - TAIL)
    for i in body[body % 7 == 0]:
        _flip_r(sig, i)
    for i in body[body % 7 == 2]:
        _flip_s(sig, i)
    for i in body[body % 7 == 4]:
        _flip_m(msg, i)
    edges = rebuilt_edges(mlen)
    row = lambda k: n - TAIL + (k + n) % TAIL  # noqa: E731
    # kind 0: untouched
    _flip_r(sig, row(1))
    _flip_s(sig, row(2))
    _flip_m(msg, row(3))
    _s_plus_l(sig, row(4))
    pk[row(5)] = undecodable_key(0xD1610000 + n)
    for k in (6, 7):
        s, a, m = edges[(n + k) % len(edges)]
        sig[row(k)], pk[row(k)], msg[row(k)] = np.frombuffer(s, np.uint8), np.frombuffer(a, np.uint8), np.frombuffer(m, np.uint8)
    return sig, pk, msg, row(5)
