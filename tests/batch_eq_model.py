"""The ZIP-215 batch equation (include/curve25519_amd.h, above ed25519_VerifyBatch_zip215_dev) in Python big integers: the expected
result and the expected point of the test hook for the CPU emulator and the GPU tests.  Decoding and curve constants come from
tests/zip215_cases.py and tests/vectors.py; the scalar multiplications use a projective addition of their own (vectors.ed_mul inverts
in every step: 0.1 s per full scalar)."""
import bisect
import hashlib

import numpy as np

from vectors import D_ED, ED_B, L, P
from zip215_cases import zip215_decode

NEUTRAL = (0, 1, 1, 0)


def _ext(p):
    return (p[0], p[1], 1, p[0] * p[1] % P)


def _add(p, q):
    """unified a = -1 addition in extended coordinates (complete on the curve)"""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a = (y1 - x1) * (y2 - x2) % P
    b = (y1 + x1) * (y2 + x2) % P
    c = 2 * D_ED * t1 * t2 % P
    d = 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def _mul(k, p):
    r = NEUTRAL
    for bit in bin(k)[2:] if k else "":
        r = _add(r, r)
        if bit == "1":
            r = _add(r, p)
    return r


def _neg(p):
    return ((P - p[0]) % P, p[1], p[2], (P - p[3]) % P)


def _affine(p):
    zi = pow(p[2], P - 2, P)
    return (p[0] * zi % P, p[1] * zi % P)


def challenge(seed, i):
    """z_i = the first 16 bytes of SHA-512(seed || le64(i)), little-endian"""
    return int.from_bytes(hashlib.sha512(seed + i.to_bytes(8, "little")).digest()[:16], "little")


def challenges(seed, n, index0=0):
    seed = bytes(seed)
    assert len(seed) == 32
    return [challenge(seed, index0 + i) for i in range(n)]


def _element(sg, key, m, z):
    """(z S, -[z]R - [z k mod L]A) of one element, or None if rules 1-3 reject it"""
    S = int.from_bytes(sg[32:], "little")
    A, R = zip215_decode(key), zip215_decode(sg[:32])
    if S >= L or A is None or R is None:
        return None
    k = int.from_bytes(hashlib.sha512(sg[:32] + key + m).digest(), "little") % L
    return z * S, _add(_neg(_mul(z, _ext(R))), _neg(_mul(z * k % L, _ext(A))))


def batch_point(sig, pk, msg, seed, index=None):
    """(T, ok): T = [sum z_i S_i mod L]B - sum [z_i]R_i - sum [z_i k_i mod L]A_i in affine coordinates over the elements that pass rules
    1-3 (the others are left out of every sum, as the hook leaves them out); ok = every element passed them.  index: the elements' own
    indices in the call (default 0 .. n - 1): the rows are then a subset of a batch, and T is that subset's share of the batch's point"""
    seed = bytes(seed)
    s_sum, acc, ok = 0, NEUTRAL, True
    for j, i in enumerate(range(len(sig)) if index is None else index):
        term = _element(bytes(sig[j]), bytes(pk[j]), bytes(msg[j]), challenge(seed, int(i)))
        if term is None:
            ok = False
            continue
        s_sum, acc = s_sum + term[0], _add(acc, term[1])
    return _affine(_add(acc, _mul(s_sum % L, _ext(ED_B)))), ok


def subset_points(sig, pk, msg, seed, index, sizes):
    """{n: the share of the rows with index[j] < n in the point of the batch's first n elements (extended coordinates)} for n in sizes:
    one pass in position order over rows that the closed form below does not cover (index ascending)"""
    seed, index = bytes(seed), [int(i) for i in index]
    assert index == sorted(index)
    out, s_sum, acc, j = {}, 0, NEUTRAL, 0
    for n in sorted(sizes):
        while j < len(index) and index[j] < n:
            term = _element(bytes(sig[j]), bytes(pk[j]), bytes(msg[j]), challenge(seed, index[j]))
            if term is not None:
                s_sum, acc = s_sum + term[0], _add(acc, term[1])
            j += 1
        out[n] = _add(acc, _mul(s_sum % L, _ext(ED_B)))
    return out


# ---- the closed form: rows whose S is moved by a known delta ----------------------------------------------------------------------
# An element that satisfies the cofactorless equation exactly ([S]B = R + [k]A) contributes the neutral element to T whatever z_i is.
# With S_i replaced by S_i + d_i mod L it contributes [z_i d_i]B (B has order L), and so does ANY element that stays in the sums, on
# top of what it contributed before.  Over rows that were exactly valid, T = [sum z_i d_i mod L]B: one SHA-512 and one multiply-add
# per element and a single scalar multiplication, at any n.  T depends on every z_i, and on every k_i (a wrong hash leaves
# [z_i (k_i' - k_i)]A_i behind).  Who knows the seed can also steer: one row's delta chosen so that the sum is 0 mod L makes the
# equation hold although no shifted element is valid.  That is the defined behaviour of a batch rule under a KNOWN seed, and the reason
# callers pass secret ones.

def shift_s(sig, rows, deltas):
    """a copy of sig[n, 64] with S of rows[j] replaced by S + deltas[j] mod L (S below L: a different value below L)"""
    buf = bytearray(np.ascontiguousarray(sig, dtype=np.uint8).tobytes())
    for r, d in zip(rows, deltas):
        at = 64 * int(r) + 32
        S = int.from_bytes(buf[at:at + 32], "little")
        assert S < L and d % L != 0, (r, d)
        buf[at:at + 32] = ((S + d) % L).to_bytes(32, "little")
    return np.frombuffer(buf, np.uint8).reshape(-1, 64)


def shift_sums(seed, rows, deltas):
    """(rows, sums): sums[k] = sum over j < k of z_rows[j] * deltas[j] (an integer, not reduced), rows ascending -- one pass over the
    challenges that every size of a test shares.  A row that rules 1-3 reject is left out of the hook's sums: leave it out here."""
    seed, rows = bytes(seed), [int(r) for r in rows]
    assert len(seed) == 32 and len(rows) == len(deltas) and all(a < b for a, b in zip(rows, rows[1:]))
    sums, total = [0], 0
    for r, d in zip(rows, deltas):
        total += challenge(seed, r) * int(d)
        sums.append(total)
    return rows, sums


def shifted_total(shifts, n):
    """sum z_i d_i mod L over the shifted rows below n"""
    rows, sums = shifts
    return sums[bisect.bisect_left(rows, n)] % L


def shifted_point(shifts, n, extra=NEUTRAL):
    """the affine point of the first n elements: [sum z_i d_i mod L]B + extra (extra: the share of the rows that were not exactly valid,
    from subset_points / batch_point, extended coordinates)"""
    return _affine(_add(_mul(shifted_total(shifts, n), _ext(ED_B)), extra))


def steering_delta(seed, shifts, n, j):
    """the delta of row j < n (its own, if it is among the shifted rows, is replaced) under which sum z_i d_i = 0 mod L over the first n
    elements: the batch then satisfies the equation"""
    rows, sums = shifts
    zj = challenge(bytes(seed), j)
    k = bisect.bisect_left(rows, j)
    own = sums[k + 1] - sums[k] if k < len(rows) and rows[k] == j else 0
    assert j < n and zj % L
    return -(shifted_total(shifts, n) - own) * pow(zj, -1, L) % L


def odd_deltas(count, seed):
    """`count` odd 62-bit deltas, seeded"""
    return [int(d) | 1 for d in np.random.default_rng(seed).integers(1 << 61, 1 << 62, count, dtype=np.uint64)]


def probe_rows(n, more=(), seed=0, at_least=64, random=32):
    """the rows of an n-element batch whose S a steered-accept test moves one at a time: rows 0, 1, 62, 63, 64, n - 2, n - 1, the two
    sides of the first eight 256-lane workgroup edges of stage 1, `more` (the caller's: run boundaries of the digit passes, neighbours
    of special rows), and `random` seeded rows -- more of those if the set would hold fewer than at_least (every row, if n is smaller)"""
    rows = {0, 1, 62, 63, 64, n - 2, n - 1} | {256 * e - d for e in range(1, 9) for d in (0, 1)} | {int(r) for r in more}
    rows = {r for r in rows if 0 <= r < n}
    if n <= at_least:
        return list(range(n))
    rest = np.random.default_rng(seed).permutation(np.setdiff1d(np.arange(n), list(rows)))
    return sorted(rows | {int(r) for r in rest[:max(random, at_least - len(rows))]})


def run_boundary_rows(n_first, n_points, pts):
    """the points on both sides of the first and the last boundary between the runs of `pts` points that one workgroup of the
    count / scatter kernels takes, as (is_second_kind, index) -- points 0 .. n_first - 1 are keys, the others R's"""
    out = []
    for p in {pts, (n_points - 1) // pts * pts}:
        if 0 < p < n_points:
            out += [(q >= n_first, q - n_first if q >= n_first else q) for q in (p - 1, p)]
    return out


def encode(pt):
    return np.frombuffer((pt[1] | ((pt[0] & 1) << 255)).to_bytes(32, "little"), np.uint8)


def batch_result(sig, pk, msg, seed):
    """the `result` of ed25519_VerifyBatch_zip215_* for one equation over the whole batch"""
    if len(sig) == 0:
        return 1
    T, ok = batch_point(sig, pk, msg, seed)
    return int(ok and _affine(_mul(8, _ext(T))) == (0, 1))


def cancelling_pair(oracle, seed=0xBA7C4E0):
    """two honest signatures with S_0 + 5 and S_1 - 5: both single verdicts are 0, and a combination with all z = 1 would accept them"""
    sk = oracle.random_bytes((2, 32), seed)
    pub, priv = oracle.ed25519_keypair(sk)
    msg = oracle.random_bytes((2, 32), seed + 1)
    sig = oracle.ed25519_sign(priv, msg).copy()
    for i, delta in ((0, 5), (1, -5)):
        S = int.from_bytes(sig[i, 32:].tobytes(), "little") + delta
        assert 0 <= S < L
        sig[i, 32:] = np.frombuffer(S.to_bytes(32, "little"), np.uint8)
    return sig, pub, msg


def torsion_pair(seed=0x7085107):
    """two signatures under keys a_i*B with R_0 = r_0*B + T8 and R_1 = r_1*B - T8, S_i = r_i + h_i*a_i: each satisfies the cofactored
    equation (and not the cofactorless one), and the two torsion parts cancel in a sum with equal weights"""
    import random

    from vectors import ed_enc, ed_order8_point
    rnd = random.Random(seed)
    T8 = _ext(ed_order8_point())
    sigs, pks, msgs = [], [], []
    for j in (1, 7):
        a, r = rnd.getrandbits(252) % L, rnd.getrandbits(252) % L
        key = ed_enc(_affine(_mul(a, _ext(ED_B))))
        m = rnd.getrandbits(256).to_bytes(32, "little")
        Rb = ed_enc(_affine(_add(_mul(r, _ext(ED_B)), _mul(j, T8))))
        h = int.from_bytes(hashlib.sha512(Rb + key + m).digest(), "little") % L
        sigs.append(Rb + ((r + h * a) % L).to_bytes(32, "little"))
        pks.append(key)
        msgs.append(m)
    f = lambda rows: np.stack([np.frombuffer(x, np.uint8) for x in rows])  # noqa: E731
    return f(sigs), f(pks), f(msgs)


def undecodable():
    """a 32-byte string without a square root (the smallest such y)"""
    y = 2
    while zip215_decode(y.to_bytes(32, "little")) is not None:
        y += 1
    return np.frombuffer(y.to_bytes(32, "little"), np.uint8)
