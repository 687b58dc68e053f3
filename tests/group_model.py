"""The rules of ed25519_ScalarMult[_noclamp]_*, ed25519_ScalarMultBase[_noclamp]_*, ed25519_PointAdd_* and ed25519_PointSub_*
(include/curve25519_amd.h, "Group operations") in Python big integers, and the case set the CPU and GPU tests of those calls share.
Everything is computed from the stated rule with tests/key_model.py's decoder and tests/vectors.py's Edwards arithmetic (ed_add,
ed_enc); tests/test_group_model.py pins the result to the compiled reference.  vectors.ed_mul pays two modular exponentiations per
addition, 50-80 ms a walk, and the case set has several hundred: mul() below is the same double-and-add over the same complete
addition law in extended coordinates with one inversion at the end, 2 ms a walk, and tests/test_group_model.py holds it against
vectors.ed_mul.  [e]P is memoised per (e, point bytes) all the same: a pytest process walks each pair once however many tests ask."""
import functools
import hashlib

import numpy as np

import key_model
from key_model import MASK255, clamp
from vectors import D_ED, ED_B, L, P, ed_add, ed_enc

ZERO32 = bytes(32)
BASE = ed_enc(ED_B)
WINDOWS = (2, 3, 4)
DIGITS = {2: 129, 3: 86, 4: 65}              # signed W-bit digits of the device's recoding (csrc/ed_group.cuh)


def scalar_value(s: bytes, clamped: bool) -> int:
    """e of the rule: the scalar clamped on a copy, or its low 255 bits"""
    return int.from_bytes(clamp(s) if clamped else s, "little") & MASK255


def _ext_add(p, q):
    """the complete addition law (a = -1) on (X : Y : Z : T), T = XY / Z"""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D_ED * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return e * f % P, g * h % P, f * g % P, e * h % P


def mul(k: int, A):
    """[k]A for an affine point A: what vectors.ed_mul computes, in extended coordinates"""
    r, p = (0, 1, 1, 0), (A[0], A[1], 1, A[0] * A[1] % P)
    while k:
        if k & 1:
            r = _ext_add(r, p)
        p = _ext_add(p, p)
        k >>= 1
    zi = pow(r[2], P - 2, P)
    return r[0] * zi % P, r[1] * zi % P


@functools.lru_cache(maxsize=None)
def _walk(e: int, point: bytes):
    A = key_model.decode(point)[0]
    return None if A is None else mul(e, A)


def enc(Q) -> bytes:
    """the canonical encoding: y < p, bit 255 the parity of x (clear for x = 0)"""
    return ed_enc((Q[0] % P, Q[1] % P))


def scalarmult(s: bytes, point: bytes, clamped: bool):
    """(q bytes, ok) of ed25519_ScalarMult (clamped) / ed25519_ScalarMult_noclamp for one element"""
    Q = _walk(scalar_value(s, clamped), point)
    return (ZERO32, 0) if Q is None else (enc(Q), 1)


def scalarmult_base(s: bytes, clamped: bool) -> bytes:
    return enc(_walk(scalar_value(s, clamped), BASE))


def point_add(p: bytes, q: bytes, sub: bool):
    """(r bytes, ok) of ed25519_PointAdd / ed25519_PointSub for one element"""
    A, B = key_model.decode(p)[0], key_model.decode(q)[0]
    if A is None or B is None:
        return ZERO32, 0
    if sub:
        B = ((P - B[0]) % P, B[1])
    return enc(ed_add(A, B)), 1


def recode(e: int, w: int):
    """the signed w-bit digits of e, least significant first, as the device forms them: the fields of e + C less R"""
    r, n = 1 << (w - 1), DIGITS[w]
    c = sum(r << (w * i) for i in range(n))
    v = e + c
    assert v < 1 << (w * n), "e + C overflows the fields"
    return [((v >> (w * i)) & ((1 << w) - 1)) - r for i in range(n)]


def _rows(rows):
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows])


def _le(v: int) -> bytes:
    return int(v % 2**256).to_bytes(32, "little")


def edge_scalars():
    """the edge scalars of the case set as 32-byte strings"""
    vals = [0, 1, 2, 7, 8, L - 1, L, L + 1, 2**252, 2**254, 2**254 + 2**253, 2**255 - 19, 2**255 - 1, 2**256 - 1,
            int("77" * 32, 16), int("88" * 32, 16), int("55" * 32, 16)]
    return [_le(v) for v in vals]


def scalars(n_random=8, seed=0x6709):
    rng = np.random.default_rng(seed)
    return edge_scalars() + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n_random)]


@functools.lru_cache(maxsize=None)
def _case_pairs():
    keys, labels = key_model.case_set()
    by = {}
    for k, lab in zip(keys, labels):
        by.setdefault(lab, []).append(k.tobytes())
    sc, pt, lab = [], [], []
    for i, s in enumerate(scalars()):
        sc.append(s); pt.append(BASE); lab.append("base point")
        for name in sorted(by):
            sc.append(s); pt.append(by[name][i % len(by[name])]); lab.append(name)
    return _rows(sc), _rows(pt), tuple(lab)


def case_set():
    """(scalars uint8[n, 32], points uint8[n, 32], labels): every scalar of scalars() -- the edge values and seeded random ones --
    paired with the base point and with one point of every label of key_model.case_set(), a different one for every scalar"""
    sc, pt, lab = _case_pairs()
    return sc.copy(), pt.copy(), list(lab)


def expected_scalarmult(sc, pt, clamped):
    """(q uint8[n, 32], ok int32[n]) of the model"""
    out = [scalarmult(bytes(s), bytes(p), clamped) for s, p in zip(sc, pt)]
    return _rows([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def expected_base(sc, clamped):
    return _rows([scalarmult_base(bytes(s), clamped) for s in sc])


def expected_add(p, q, sub):
    out = [point_add(bytes(a), bytes(b), sub) for a, b in zip(p, q)]
    return _rows([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


@functools.lru_cache(maxsize=None)
def _add_pairs():
    keys, labels = key_model.case_set()
    lab = np.array(labels)
    rows = [k.tobytes() for k in keys]
    neg = lambda k: k[:31] + bytes([k[31] ^ 0x80])          # noqa: E731  (-x: the other sign bit; x = 0 decodes either way)
    p, q, names = [], [], []
    for i, k in enumerate(rows):                           # every case point with its neighbour, itself and its negative
        for other, name in ((rows[(i + 1) % len(rows)], "next"), (k, "P + P"), (neg(k), "P + (-P)")):
            p.append(k); q.append(other); names.append(f"{labels[i]} / {name}")
    small = [rows[i] for i in np.flatnonzero(lab == "small order")]
    for a in small:                                        # torsion + torsion
        for b in small:
            p.append(a); q.append(b); names.append("torsion / torsion")
    return _rows(p), _rows(q), tuple(names)


def add_cases():
    """(p uint8[n, 32], q uint8[n, 32], labels): every point of key_model.case_set() with the next one, with itself and with its
    negative, and every pair of small-order encodings"""
    p, q, names = _add_pairs()
    return p.copy(), q.copy(), list(names)


def montgomery_u_of(q: bytes) -> bytes:
    """u = (1 + y) / (1 - y) of an encoded point, 32 bytes (0 for y = 1)"""
    return key_model.montgomery_u(int.from_bytes(q, "little") & MASK255).to_bytes(32, "little")


def seed_scalar(seed: bytes) -> bytes:
    """clamp(SHA-512(seed)[0..31]): the scalar of the key pair made from `seed`"""
    return clamp(hashlib.sha512(seed).digest())

