"""The strict verification rule (include/curve25519_amd.h, above ed25519_VerifySignature_strict_batch) in Python big integers, and the
edge set the CPU and GPU tests of the strict calls share.  The rule's rule 6 is the reference's verdict, which the caller passes in
(the oracle's, or tests/golden/degenerate_verify.npz's): nothing here decides whether a signature equation holds."""
import hashlib

import numpy as np

from vectors import L, P, ED_B, ed_add, ed_decode, ed_enc, ed_mul, ed_order8_point, small_order_encodings, torsion_signature_cases

MASK255 = 2**255 - 1
SMALL_Y = frozenset(ed_mul(k, ed_order8_point())[1] for k in range(8))      # 0, 1, p - 1, y8, p - y8


def _int(row):
    return int.from_bytes(bytes(row), "little")


def strict_rule(sig, pk, ref):
    """int32[n]: ref[i] where element i keeps rules 1-5, else 0"""
    out = np.zeros(len(sig), np.int32)
    for i in range(len(sig)):
        S, yR, a = _int(sig[i][32:]), _int(sig[i][:32]) & MASK255, _int(pk[i])
        yA = a & MASK255
        ok = S < L and yA < P and yA % P not in SMALL_Y and ed_decode(yA, a >> 255) is not None and yR % P not in SMALL_Y
        out[i] = int(ref[i]) if ok else 0
    return out


def _le(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def predicate_values():
    """32-byte values around every boundary the predicates draw: L, p and the small-order y, with bit 255 set and clear"""
    vals = {0, 1, 2, L - 1, L, L + 1, 2**252 - 1, 2**252, 2**252 + 1, 2**255 - 1, 2**256 - 1, P - 2, P - 1, P, P + 1, P + 2}
    for y in SMALL_Y:
        vals |= {y - 1, y, y + 1}
    vals |= {v | 2**255 for v in list(vals)}
    return np.stack([_le(v % 2**256) for v in sorted(vals)])


def _sign_with(a, t, pk_bytes, m, rnd):
    """(R, S) that satisfy the cofactorless equation for the key a*B + t*T8 under the 32 bytes pk_bytes: R = r*B + j*T8 with
    j + h*t = 0 mod 8 (tests/vectors.py: torsion_signature_cases), S = r + h*a mod L"""
    T8 = ed_order8_point()
    while True:
        r = rnd.getrandbits(256) % L
        for j in range(8):
            Rb = ed_enc(ed_add(ed_mul(r, ED_B), ed_mul(j, T8)))
            h = int.from_bytes(hashlib.sha512(Rb + pk_bytes + m).digest(), "little") % L
            if (j + h * t) % 8 == 0:
                return Rb, (r + h * a) % L


def edge_cases(oracle, seed=5):
    """(sig[n, 64], pk[n, 32], msg[n, 32]): honest and corrupted signatures, S in {L - 1, L, L + 1, S + L, 2^252 +- 1, 2^256 - 1},
    every small-order encoding as key and as R, keys with y in [p, 2^255) and both sign bits, x = 0 with the sign bit, keys off
    the curve, mixed-order keys with correct signatures"""
    import random
    rnd = random.Random(seed)
    sk = oracle.random_bytes((16, 32), 0x5721C7 + seed)
    pub, priv = oracle.ed25519_keypair(sk)
    msg = oracle.random_bytes((16, 32), 0x5721C8 + seed)
    honest = oracle.ed25519_sign(priv, msg)
    sigs, pks, msgs = [], [], []

    def put(sig, pk, m):
        sigs.append(np.frombuffer(bytes(sig), np.uint8))
        pks.append(np.frombuffer(bytes(pk), np.uint8))
        msgs.append(np.frombuffer(bytes(m), np.uint8))

    for i in range(16):
        s, pk, m = honest[i].tobytes(), pub[i].tobytes(), msg[i].tobytes()
        S = _int(s[32:])
        put(s, pk, m)                                                            # honest
        put(s[:32] + ((S + L) % 2**256).to_bytes(32, "little"), pk, m)          # S + L
        bad = bytearray(s)
        bad[i % 64] ^= 1 << (i % 8)
        put(bad, pk, m)                                                          # corrupted
        bad = bytearray(m)
        bad[i] ^= 0x80
        put(s, pk, bad)                                                          # another message
        for v in (L - 1, L, L + 1, 2**252 - 1, 2**252 + 1, 2**256 - 1):
            put(s[:32] + v.to_bytes(32, "little"), pk, m)
    for enc, _ in small_order_encodings():
        put(honest[0].tobytes(), enc, msg[0].tobytes())                          # a small-order key
        put(enc + honest[1].tobytes()[32:], pub[1].tobytes(), msg[1].tobytes())  # a small-order R
    for y in list(range(P, 2**255)) + [1, P - 1]:
        for sign in (0, 1):
            put(honest[2].tobytes(), (y | (sign << 255)).to_bytes(32, "little"), msg[2].tobytes())
    off = [y for y in range(2, 64) if ed_decode(y, 0) is None][:6]
    for y in off:
        for sign in (0, 1):
            put(honest[3].tobytes(), (y | (sign << 255)).to_bytes(32, "little"), msg[3].tobytes())
    # keys of every class with a signature whose equation holds: a*B + t*T8 (mixed order), y >= p encodings of honest keys
    T8 = ed_order8_point()
    for t in range(8):
        a = rnd.getrandbits(252) % L
        A = ed_enc(ed_add(ed_mul(a, ED_B), ed_mul(t, T8)))
        m = rnd.getrandbits(256).to_bytes(32, "little")
        for _ in range(2):
            Rb, S = _sign_with(a, t, A, m, rnd)
            put(Rb + S.to_bytes(32, "little"), A, m)
            put(Rb + (S + L).to_bytes(32, "little"), A, m)
    tsig, tpk, tmsg = torsion_signature_cases(count=3, seed=seed)
    for i in range(len(tsig)):
        put(tsig[i], tpk[i], tmsg[i])
    return np.stack(sigs), np.stack(pks), np.stack(msgs)


def hostile(sig, pk, kind):
    """copies of honest (sig, pk) with every second key off the curve ('offcurve'), every S replaced by S + L ('s_plus_l') or every
    key of small order ('small_key')"""
    sig, pk = sig.copy(), pk.copy()
    if kind == "offcurve":
        y = next(y for y in range(2, 64) if ed_decode(y, 0) is None)
        pk[1::2] = _le(y)
    elif kind == "s_plus_l":
        S = sig[:, 32:].astype(np.uint64).copy()
        carry = np.zeros(len(sig), np.uint64)
        Lb = _le(L).astype(np.uint64)
        for j in range(32):
            t = S[:, j] + Lb[j] + carry
            sig[:, 32 + j] = (t & 0xFF).astype(np.uint8)
            carry = t >> 8
    elif kind == "small_key":
        encs = [e for e, _ in small_order_encodings()]
        pk[:] = np.stack([np.frombuffer(encs[i % len(encs)], np.uint8) for i in range(len(pk))])
    else:
        raise ValueError(kind)
    return sig, pk
