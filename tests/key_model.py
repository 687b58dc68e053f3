"""The rules of ed25519_ClassifyKey_*, ed25519_PublicKey_to_X25519_* and ed25519_PrivateKey_to_X25519_* (include/curve25519_amd.h) in
Python big integers, and the case set the CPU and GPU tests of those calls share.  Everything is computed from the stated rule with
tests/vectors.py's affine Edwards arithmetic: the order bits are ed_mul(8, A) and ed_mul(L, A) compared with the neutral element,
nothing is looked up.  A walk by L costs ~30 ms here, so [L]A is memoised per 32-byte string: a pytest process walks each key of
the pool once however many tests ask."""
import functools
import hashlib

import numpy as np

from strict_cases import predicate_values
from vectors import L, P, ed_add, ed_decode, ed_enc, ed_mul, ed_order8_point, small_order_encodings

DECODES, CANONICAL, SMALL_ORDER, TORSION_FREE = 1, 2, 4, 8
MASK255 = 2**255 - 1
NEUTRAL = (0, 1)


def decode(key: bytes):
    """(A, y, sign): A the point the 32 bytes decode to under the ZIP-215 rule, or None"""
    v = int.from_bytes(key, "little")
    y, sign = v & MASK255, v >> 255
    A = ed_decode(y % P, sign)               # x = 0 decodes whatever the sign bit says (P - 0 is 0 mod p)
    return (None if A is None else (A[0] % P, A[1])), y, sign


@functools.lru_cache(maxsize=None)
def times_L(key: bytes):
    """[L]A for the point the key decodes to (None where it does not decode)"""
    A = decode(key)[0]
    return None if A is None else ed_mul(L, A)


def classify(key: bytes) -> int:
    """the flags of one 32-byte key"""
    A, y, sign = decode(key)
    flags = 0
    if A is not None:
        flags |= DECODES
    if y < P and not (A is not None and A[0] == 0 and sign == 1):
        flags |= CANONICAL
    if A is not None and ed_mul(8, A) == NEUTRAL:
        flags |= SMALL_ORDER
    if A is not None and times_L(key) == NEUTRAL:
        flags |= TORSION_FREE
    return flags


def montgomery_u(y: int) -> int:
    """u = (1 + y) / (1 - y) mod p (0 for y = 1)"""
    y %= P
    return (1 + y) * pow((1 - y) % P, P - 2, P) % P


def to_x25519(key: bytes):
    """(xpk bytes, ok) of ed25519_PublicKey_to_X25519 for one key"""
    if classify(key) & (DECODES | SMALL_ORDER | TORSION_FREE) != (DECODES | TORSION_FREE):
        return bytes(32), 0
    return montgomery_u(int.from_bytes(key, "little") & MASK255).to_bytes(32, "little"), 1


def clamp(b: bytes) -> bytes:
    a = bytearray(b[:32])
    a[0] &= 248
    a[31] &= 127
    a[31] |= 64
    return bytes(a)


def private_to_x25519(priv: bytes) -> bytes:
    """xsk of ed25519_PrivateKey_to_X25519 for one 64-byte privKey (seed || pk): the seed half alone is read"""
    return clamp(hashlib.sha512(priv[:32]).digest())


def _rows(keys):
    return np.stack([np.frombuffer(bytes(k), np.uint8) for k in keys])


def expected(keys):
    """(flags uint32[n], xpk uint8[n, 32], ok int32[n]) of the model for uint8[n, 32] keys"""
    flags = np.array([classify(bytes(k)) for k in keys], np.uint32)
    conv = [to_x25519(bytes(k)) for k in keys]
    return flags, _rows([c[0] for c in conv]), np.array([c[1] for c in conv], np.int32)


def _le(v: int) -> bytes:
    return int(v).to_bytes(32, "little")


def _flip_sign(key: bytes) -> bytes:
    return key[:31] + bytes([key[31] ^ 0x80])


def off_curve_y(count=12):
    """the first `count` y >= 2 for which (y^2 - 1) / (d y^2 + 1) has no square root, and as many counted down from p - 2"""
    lo, hi, y = [], [], 2
    while len(lo) < count // 2:
        if ed_decode(y, 0) is None:
            lo.append(y)
        y += 1
    y = P - 2
    while len(hi) < count - count // 2:
        if ed_decode(y, 0) is None:
            hi.append(y)
        y -= 1
    return lo + hi


def honest_keys(oracle, count, seed=0xED25):
    """(pub uint8[count, 32], priv uint8[count, 64]) from the oracle's ed25519_keypair on seeded secrets"""
    from curve25519_amd import synth
    return oracle.ed25519_keypair(synth.random_bytes((count, 32), seed))


def mixed_order_keys(pub):
    """for each honest key A and each of the seven non-zero 8-torsion points T: enc(A + T), of order 2L, 4L or 8L"""
    T8 = ed_order8_point()
    torsion = [ed_mul(k, T8) for k in range(1, 8)]
    out = []
    for row in pub:
        v = int.from_bytes(bytes(row), "little")
        A = ed_decode(v & MASK255, v >> 255)
        assert A is not None
        out += [ed_enc(ed_add(A, T)) for T in torsion]
    return out


@functools.lru_cache(maxsize=None)
def _case_keys(n_honest):
    from oracle_lib import Oracle
    pub, _ = honest_keys(Oracle(), n_honest)
    keys, labels = [], []

    def put(label, rows):
        for r in rows:
            keys.append(bytes(r))
            labels.append(label)

    put("honest", [bytes(r) for r in pub])
    put("honest negated", [_flip_sign(bytes(r)) for r in pub])
    put("mixed order", mixed_order_keys(pub))
    put("small order", [e for e, _ in small_order_encodings()])
    put("y >= p", [_le((P + k) | (s << 255)) for k in range(19) for s in (0, 1)])
    put("x = 0 with the sign bit", [_le(y | (1 << 255)) for y in (P - 1, P, P + 1)])
    put("off the curve", [_le(y | (s << 255)) for i, y in enumerate(off_curve_y(12)) for s in (i & 1,)])
    put("predicate boundary", [bytes(r) for r in predicate_values()])
    return _rows(keys), tuple(labels)


def case_set(n_honest=6):
    """(keys uint8[n, 32], labels): the shared edge set -- honest keys and their negations, every honest key shifted by every non-zero
    8-torsion point, the 14 small-order encodings, y = p .. p + 18 with both sign bits, x = 0 with the sign bit, y off the curve and
    the strict predicates' boundary values"""
    keys, labels = _case_keys(n_honest)
    return keys.copy(), list(labels)


def pool(n_extra=12):
    """about 300 modelled keys for the size tests: the case set, then more honest keys and their mixed-order shifts"""
    from oracle_lib import Oracle
    keys, _ = case_set()
    pub, _ = honest_keys(Oracle(), n_extra, seed=0xED26)
    extra = [bytes(r) for r in pub] + [_flip_sign(bytes(r)) for r in pub] + mixed_order_keys(pub)
    return np.concatenate([keys, _rows(extra)])
