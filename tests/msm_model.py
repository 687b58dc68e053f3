"""The rules of ed25519_MultiScalarMult[_vartime]_* and ristretto255_MultiScalarMult[_vartime]_* (include/curve25519_amd.h,
"multiscalar multiplication") in Python big integers, on top of tests/group_model.py and tests/ristretto_model.py, and the cases the
CPU and GPU tests of those calls share.  It is never the library under test.

A group's sum is Q = sum_i [s_i mod L] P_i.  To keep the model fast at any m every case draws its points from a pool of at most 16
distinct encodings, and the expected sum is sum_j [sum_{i: P_i = pool_j} (s_i mod L)] pool_j with the inner sum an INTEGER (not reduced
again: the Edwards pool holds points with a torsion part, on which [k]P and [k mod L]P differ): at most 16 big-integer walks per group
whatever m is.  The kernels see no structure in it; the repeated points put equal points into one bucket and one chunk, which is what
the complete additions are claimed to handle."""
import functools

import numpy as np

import group_model
import key_model
import ristretto_model
from vectors import ED_B, L, P, ed_add, ed_enc, ed_order8_point

GROUPS = ("ed25519", "ristretto255")
ZERO32 = bytes(32)
SUM_CHUNK = 64                             # csrc/msm_sum.cuh: MSM_SUM_CHUNK
WIDTHS = tuple(range(7, 14))               # csrc/msm25519.cuh: MSM_C_MIN .. MSM_C_MAX
IDENTITY = {"ed25519": (1).to_bytes(32, "little"), "ristretto255": ZERO32}


def _le(v: int) -> bytes:
    return int(v % 2**256).to_bytes(32, "little")


def _rows(rows):
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows])


def decode(group: str, b: bytes):
    """the affine point the 32 bytes decode to under the group's rule, or None"""
    return key_model.decode(b)[0] if group == "ed25519" else ristretto_model.decode(b)


def encode(group: str, A) -> bytes:
    return group_model.enc(A) if group == "ed25519" else ristretto_model.encode((A[0] % P, A[1] % P))


@functools.lru_cache(maxsize=None)
def pool(group: str):
    """(points that decode, {"non-decoding": bytes, "non-canonical": bytes}): at most 16 encodings in all.  Random points, B, the neutral
    element; Edwards only: a point of order 8, a mixed-order point and y = p + 1 (which ZIP-215 decodes, to the neutral element).  The
    ristretto255 non-canonical encoding is s = p + 2 (even, s - p decodes), which DECODE refuses; the Edwards one is listed for
    symmetry and is NOT a reject."""
    rng = np.random.default_rng(0x4d534d)
    ks = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % L for _ in range(8)]
    pts = [group_model.mul(k, ED_B) for k in ks]
    if group == "ed25519":
        t8 = ed_order8_point()
        good = [ed_enc(A) for A in pts] + [group_model.BASE, IDENTITY[group], ed_enc(t8), ed_enc(ed_add(pts[0], t8)), _le(P + 1)]
        bad = key_model._le(key_model.off_curve_y(2)[0])
        rejects = {"non-decoding": bad, "non-canonical": _le(P + 1)}
    else:
        good = [ristretto_model.encode(A) for A in pts] + [ristretto_model.BASE, IDENTITY[group]]
        s = 3
        while ristretto_model.decode_why(_le(s))[1] != "not square":
            s += 1
        rejects = {"non-decoding": _le(s), "non-canonical": _le(P + 2)}
        assert ristretto_model.decode_why(rejects["non-canonical"])[1] == "non-canonical"
    assert all(decode(group, g) is not None for g in good) and decode(group, rejects["non-decoding"]) is None
    assert len(set(good)) + 2 <= 16
    return tuple(good), rejects


def expected_group(group: str, scalars, points):
    """(q bytes, ok) of one group: scalars and points are sequences of 32-byte strings"""
    total = {}
    for s, p in zip(scalars, points):
        total[bytes(p)] = total.get(bytes(p), 0) + int.from_bytes(bytes(s), "little") % L
    assert len(total) <= 16, "a case draws from the pool"
    Q = (0, 1)
    for p, k in total.items():
        A = decode(group, p)
        if A is None:
            return ZERO32, 0
        Q = ed_add(Q, group_model.mul(k, A))
    return encode(group, Q), 1


def expected(group: str, sc, pt, m: int):
    """(q uint8[n_groups, 32], ok int32[n_groups]) for scalar and point arrays uint8[n_groups * m, 32]"""
    assert len(sc) == len(pt) and len(sc) % m == 0
    out = [expected_group(group, [bytes(r) for r in sc[g:g + m]], [bytes(r) for r in pt[g:g + m]]) for g in range(0, len(sc), m)]
    return _rows([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


EDGE_SCALARS = tuple(_le(v) for v in (0, 1, L - 1, L, L + 1, 2**252, 2**255 - 1, 2**256 - 1))


def window_scalars(c: int):
    """scalars below 2^252 (canonical as they stand) whose c-bit windows are all 0, all 2^(c-1) and all 2^c - 1 as far as they reach"""
    full = range(252 // c)
    return [_le(0), _le(sum(1 << (c * w + c - 1) for w in full)), _le(sum(((1 << c) - 1) << (c * w) for w in full))]


def scalar_set(seed: int, n_random=8):
    """the edge scalars, every width's window patterns and seeded random 256-bit strings"""
    rng = np.random.default_rng(seed)
    out = list(EDGE_SCALARS)
    for c in WIDTHS:
        out += window_scalars(c)[1:]
    return out + [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n_random)]


def case(group: str, n_groups: int, m: int, seed=1, kind="mixed"):
    """(scalar uint8[n_groups * m, 32], point uint8[n_groups * m, 32]) with points drawn from the pool's decoding half.  kind:
    "mixed" -- scalars cycle through scalar_set in a seeded order; "equal" -- one random scalar everywhere (one long bucket list, the
    split top window); "cancel" -- m is even and rows 2 i, 2 i + 1 are s P, (L - s) P: every group sums to the identity"""
    rng = np.random.default_rng([seed, n_groups, m, GROUPS.index(group)])
    good, _ = pool(group)
    rows = n_groups * m
    pts = [good[i] for i in rng.integers(0, len(good), rows)]
    if kind == "mixed":
        ss = scalar_set(seed)
        start = int(rng.integers(0, len(ss)))
        scs = [ss[(start + 7 * i) % len(ss)] for i in range(rows)]
    elif kind == "equal":
        scs = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes()] * rows
    elif kind == "cancel":
        assert m % 2 == 0
        scs = []
        for i in range(0, rows, 2):                        # (points of order L: the random ones and B)
            s = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % L
            scs += [_le(s), _le(L - s)]
            pts[i] = pts[i + 1] = good[int(rng.integers(0, 9))]
    else:
        raise ValueError(kind)
    return _rows(scs), _rows(pts)


def with_reject(group: str, pt, row: int, which="non-decoding"):
    """a copy of the point array with the pool's reject encoding in `row`"""
    out = pt.copy()
    out[row] = np.frombuffer(pool(group)[1][which], np.uint8)
    return out


DEFAULT_SHAPES = ((1, 1), (1, 2), (3, 1), (5, 7), (1, 63), (1, 64), (1, 65), (2, 4097), (65, 3), (257, 2))   # (n_groups, m)
BUCKET_M = (1, 2, 65, 300)
