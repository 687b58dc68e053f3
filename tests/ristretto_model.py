"""ristretto255 (RFC 9496) in Python big integers: DECODE (4.3.1), ENCODE (4.3.2) and the Elligator MAP behind hash-to-group (4.3.4),
written in the RFC's operation order, and the rules of the ristretto255_* calls (include/curve25519_amd.h, "ristretto255") on top
of them.  tests/test_ristretto_model.py pins the model to the RFC's published vectors; the host-emulation and GPU tests compare the
lane code with it byte for byte on the case set below.  The scalar multiplication is tests/group_model.py's walk on the decoded
point; nothing here reads the device code's constants."""
import functools
import hashlib

import numpy as np

import group_model
from vectors import D_ED as D, ED_B, L, P

ZERO32 = bytes(32)
MASK255 = (1 << 255) - 1
SQRT_M1 = pow(2, (P - 1) // 4, P)
WINDOWS = group_model.WINDOWS


def _is_neg(x: int) -> bool:
    return bool(x % P & 1)


def _abs(x: int) -> int:
    x %= P
    return P - x if x & 1 else x


def _root_of(v: int) -> int:
    """a square root of v (v a square)"""
    r = pow(v, (P + 3) // 8, P)
    if r * r % P != v % P:
        r = r * SQRT_M1 % P
    assert r * r % P == v % P
    return r


# the constants of RFC 9496 section 4.1, derived from d
INVSQRT_A_MINUS_D = _abs(pow(_root_of(-1 - D), P - 2, P))
SQRT_AD_MINUS_ONE = P - _abs(_root_of(-D - 1))                   # the odd ("negative") root
ONE_MINUS_D_SQ = (1 - D * D) % P
D_MINUS_ONE_SQ = (D - 1) ** 2 % P


def sqrt_ratio_m1(u: int, v: int):
    """(was_square, r) of SQRT_RATIO_M1: the non-negative root of u / v, or of SQRT_M1 * u / v where there is none"""
    r = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    check = v * r * r % P
    correct = check == u % P
    flipped = check == -u % P
    flipped_i = check == -u * SQRT_M1 % P
    if flipped or flipped_i:
        r = r * SQRT_M1 % P
    return correct or flipped, _abs(r)


def decode_why(b: bytes):
    """((x, y) or None, class) of DECODE: class is "valid", "non-canonical", "negative s", "not square", "negative t" or "y = 0" """
    s = int.from_bytes(b, "little")
    if s >= P:
        return None, "non-canonical"
    if s & 1:
        return None, "negative s"
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(D * u1 * u1) - u2_sqr) % P
    was_square, invsqrt = sqrt_ratio_m1(1, v * u2_sqr % P)
    den_x = invsqrt * u2 % P
    den_y = invsqrt * den_x * v % P
    x = _abs(2 * s * den_x)
    y = u1 * den_y % P
    t = x * y % P
    if not was_square:
        return None, "not square"
    if _is_neg(t):
        return None, "negative t"
    if y == 0:
        return None, "y = 0"
    return (x, y), "valid"


def decode(b: bytes):
    return decode_why(b)[0]


def encode_ext(x0: int, y0: int, z0: int, t0: int):
    """(32 bytes, rotate) of ENCODE for an extended point"""
    u1 = (z0 + y0) * (z0 - y0) % P
    u2 = x0 * y0 % P
    _, invsqrt = sqrt_ratio_m1(1, u1 * u2 * u2 % P)
    den1, den2 = invsqrt * u1 % P, invsqrt * u2 % P
    z_inv = den1 * den2 * t0 % P
    ix0, iy0 = x0 * SQRT_M1 % P, y0 * SQRT_M1 % P
    enchanted = den1 * INVSQRT_A_MINUS_D % P
    rotate = _is_neg(t0 * z_inv)
    x, y, den_inv = (iy0, ix0, enchanted) if rotate else (x0, y0, den2)
    if _is_neg(x * z_inv):
        y = -y % P
    return _abs(den_inv * (z0 - y)).to_bytes(32, "little"), rotate


def encode(A) -> bytes:
    """ENCODE of an affine point"""
    return encode_ext(A[0], A[1], 1, A[0] * A[1] % P)[0]


def encode_rotates(A) -> bool:
    return encode_ext(A[0], A[1], 1, A[0] * A[1] % P)[1]


def elligator_map(t: int):
    """((X, Y, Z, T), was_square) of MAP"""
    r = SQRT_M1 * t * t % P
    u = (r + 1) * ONE_MINUS_D_SQ % P
    v = (-1 - r * D) * (r + D) % P
    was_square, s = sqrt_ratio_m1(u, v)
    s_prime = -_abs(s * t) % P
    s = s if was_square else s_prime
    c = P - 1 if was_square else r
    n = (c * (r - 1) * D_MINUS_ONE_SQ - v) % P
    w0, w1, w2, w3 = 2 * s * v % P, n * SQRT_AD_MINUS_ONE % P, (1 - s * s) % P, (1 + s * s) % P
    return (w0 * w3 % P, w2 * w1 % P, w1 * w3 % P, w0 * w2 % P), was_square


def hash_halves(h: bytes):
    """the two field elements of a 64-byte string: each half little-endian, bit 255 masked, mod p"""
    return [(int.from_bytes(h[i:i + 32], "little") & MASK255) % P for i in (0, 32)]


def from_hash(h: bytes) -> bytes:
    """ristretto255_FromHash for one element: ENCODE(MAP(low half) + MAP(high half))"""
    (p1, _), (p2, _) = (elligator_map(t) for t in hash_halves(h))
    return encode_ext(*group_model._ext_add(p1, p2))[0]


def from_hash_rotates(h: bytes) -> bool:
    """whether ENCODE rotates the sum of the two MAPs (the representative the device encodes too)"""
    (p1, _), (p2, _) = (elligator_map(t) for t in hash_halves(h))
    return encode_ext(*group_model._ext_add(p1, p2))[1]


def hash_squares(h: bytes):
    """was_square of the two MAPs of a 64-byte string"""
    return tuple(elligator_map(t)[1] for t in hash_halves(h))


def is_valid_point(b: bytes) -> int:
    return 0 if decode(b) is None else 1


def scalar_value(s: bytes) -> int:
    """e of the rule: the low 255 bits, no clamp"""
    return int.from_bytes(s, "little") & MASK255


@functools.lru_cache(maxsize=None)
def _walk(e: int, point: bytes):
    A = decode(point)
    return None if A is None else encode(group_model.mul(e, A))


def scalarmult(s: bytes, point: bytes):
    """(q bytes, ok) of ristretto255_ScalarMult for one element"""
    q = _walk(scalar_value(s), point)
    return (ZERO32, 0) if q is None else (q, 1)


BASE = encode(ED_B)


def scalarmult_base(s: bytes) -> bytes:
    return _walk(scalar_value(s), BASE)


def point_add(p: bytes, q: bytes, sub: bool):
    """(r bytes, ok) of ristretto255_PointAdd / PointSub for one element"""
    A, B = decode(p), decode(q)
    if A is None or B is None:
        return ZERO32, 0
    if sub:
        B = ((P - B[0]) % P, B[1])
    return encode(group_model.ed_add(A, B)), 1


# ---- the case set ------------------------------------------------------------------------------------------------------------
def _le(v: int) -> bytes:
    return int(v).to_bytes(32, "little")


FIXED_REJECTS = (
    (bytes([0]) + bytes([0xff]) * 31, "non-canonical"),
    (bytes([0xf3]) + bytes([0xff]) * 30 + bytes([0x7f]), "non-canonical"),
    (bytes([0xed]) + bytes([0xff]) * 30 + bytes([0x7f]), "non-canonical"),
    (bytes([1]) + bytes(31), "negative s"),
    (bytes([0xec]) + bytes([0xff]) * 30 + bytes([0x7f]), "y = 0"),
)


def _rows(rows):
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows])


@functools.lru_cache(maxsize=None)
def _hashes(n_random=64, seed=0x9496):
    rng = np.random.default_rng(seed)
    rows = [bytes(64), bytes([0xff]) * 64, hashlib.sha512(b"Ristretto is traditionally a short shot of espresso coffee").digest(),
            _le(P) + _le(P - 1), _le(1) + _le(2**255 + 1), _le(P + 18) + _le(2**256 - 1)]
    rows += [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(n_random)]
    return tuple(rows)


def hashes():
    """uint8[n, 64]: edge strings (zeros, ones, the RFC's vector, halves at and above p, bit 255 set) and seeded random ones"""
    return _rows(_hashes())


@functools.lru_cache(maxsize=None)
def _points(n_random=96, seed=0x4317):
    rng = np.random.default_rng(seed)
    rows, labels = [], []
    for b, why in FIXED_REJECTS:
        rows.append(b); labels.append(why)
    rows.append(ZERO32); labels.append("valid")                  # the identity
    for k in (1, 2, 3, 4, L - 1):
        rows.append(encode(group_model.mul(k, ED_B))); labels.append("valid")
    for h in _hashes()[:24]:
        rows.append(from_hash(h)); labels.append("valid")
    for _ in range(n_random):                                    # random even canonical s: every decode class turns up
        s = (int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") & MASK255) % P & ~1
        rows.append(_le(s)); labels.append(decode_why(_le(s))[1])
    rows.append(_le(2**255 + 2)); labels.append("non-canonical")  # bit 255 set on an otherwise fine s
    return tuple(rows), tuple(labels)


def points():
    """(uint8[n, 32], labels): the five fixed rejects, the identity, generator multiples, FromHash outputs and seeded random even
    canonical s, each labelled with its decode class"""
    rows, labels = _points()
    return _rows(rows), list(labels)


def scalars(n_random=8, seed=0x6710):
    rng = np.random.default_rng(seed)
    return group_model.edge_scalars() + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n_random)]


@functools.lru_cache(maxsize=None)
def _case_pairs():
    rows, labels = _points()
    by = {}
    for r, lab in zip(rows, labels):
        by.setdefault(lab, []).append(r)
    sc, pt, lab = [], [], []
    for i, s in enumerate(scalars()):
        sc.append(s); pt.append(BASE); lab.append("base point")
        for name in sorted(by):
            for j in range(4 if name == "valid" else 1):
                k = 4 * i + j if name == "valid" else i
                sc.append(s); pt.append(by[name][k % len(by[name])]); lab.append(name)
    return _rows(sc), _rows(pt), tuple(lab)


def case_set():
    """(scalars uint8[n, 32], points uint8[n, 32], labels): every scalar of scalars() -- group_model.edge_scalars() and seeded random
    ones -- with the generator, four valid points and one point of every other decode class, different ones for every scalar"""
    sc, pt, lab = _case_pairs()
    return sc.copy(), pt.copy(), list(lab)


@functools.lru_cache(maxsize=None)
def _add_pairs():
    rows, labels = _points()
    p, q, names = [], [], []
    for i, k in enumerate(rows):                                 # every point with its neighbour and with itself
        for other, name in ((rows[(i + 1) % len(rows)], "next"), (k, "P, P")):
            p.append(k); q.append(other); names.append(f"{labels[i]} / {name}")
    return _rows(p), _rows(q), tuple(names)


def add_cases():
    p, q, names = _add_pairs()
    return p.copy(), q.copy(), list(names)


def expected_valid(pt):
    return np.array([is_valid_point(bytes(p)) for p in pt], np.int32)


def expected_from_hash(h):
    return _rows([from_hash(bytes(x)) for x in h])


def expected_scalarmult(sc, pt):
    out = [scalarmult(bytes(s), bytes(p)) for s, p in zip(sc, pt)]
    return _rows([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def expected_base(sc):
    return _rows([scalarmult_base(bytes(s)) for s in sc])


def expected_add(p, q, sub):
    out = [point_add(bytes(a), bytes(b), sub) for a, b in zip(p, q)]
    return _rows([o[0] for o in out]), np.array([o[1] for o in out], np.int32)
