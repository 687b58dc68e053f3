"""The ZIP-215 batch equation (include/curve25519_amd.h, above ed25519_VerifyBatch_zip215_dev) in Python big integers: the expected
result and the expected point of the test hook for the CPU emulator and the GPU tests.  Decoding and curve constants come from
tests/zip215_cases.py and tests/vectors.py; the scalar multiplications use a projective addition of their own (vectors.ed_mul inverts
in every step: 0.1 s per full scalar)."""
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


def challenges(seed, n, index0=0):
    """z_i = the first 16 bytes of SHA-512(seed || le64(i)), little-endian"""
    seed = bytes(seed)
    assert len(seed) == 32
    return [int.from_bytes(hashlib.sha512(seed + (index0 + i).to_bytes(8, "little")).digest()[:16], "little") for i in range(n)]


def batch_point(sig, pk, msg, seed):
    """(T, ok): T = [sum z_i S_i mod L]B - sum [z_i]R_i - sum [z_i k_i mod L]A_i in affine coordinates over the elements that pass rules
    1-3 (the others are left out of every sum, as the hook leaves them out); ok = every element passed them"""
    n = len(sig)
    z = challenges(seed, n)
    s_sum, acc, ok = 0, NEUTRAL, True
    for i in range(n):
        sg, key, m = bytes(sig[i]), bytes(pk[i]), bytes(msg[i])
        S = int.from_bytes(sg[32:], "little")
        A, R = zip215_decode(key), zip215_decode(sg[:32])
        if S >= L or A is None or R is None:
            ok = False
            continue
        k = int.from_bytes(hashlib.sha512(sg[:32] + key + m).digest(), "little") % L
        s_sum = (s_sum + z[i] * S) % L
        acc = _add(acc, _neg(_mul(z[i], _ext(R))))
        acc = _add(acc, _neg(_mul(z[i] * k % L, _ext(A))))
    return _affine(_add(acc, _mul(s_sum, _ext(ED_B)))), ok


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
