"""Big-integer model of the scalar calls (ed25519_ScalarReduce_*, _ScalarAdd_*, _ScalarSub_*, _ScalarMul_*, _ScalarNegate_*,
_ScalarComplement_*, _ScalarMulAdd_*, _ScalarInvert_*, _ScalarIsCanonical_*: include/curve25519_amd.h) and the case set the CPU and
GPU tests share.  Every input is any 32-byte value (ScalarReduce: 64 bytes) and stands for its value mod L; every output is the
canonical representative in [0, L).  The model is Python's % and pow(x, -1, L); tests/test_scalar_model.py pins it to fixed vectors."""
import functools

import numpy as np

L = 2**252 + 27742317777372353535851937790883648493
KS = (1, 2, 4, 8, 16)                 # the group sizes k_sc25519_invert is instantiated for (tunable SC_INVERT_K)


def reduce(x):
    return x % L


def add(x, y):
    return (x + y) % L


def sub(x, y):
    return (x - y) % L


def mul(x, y):
    return x * y % L


def negate(x):
    return -x % L


def complement(x):
    return (1 - x) % L


def muladd(a, b, c):
    return (a * b + c) % L


def invert(x):
    """(1 / x mod L, 1), or (0, 0) where x mod L == 0: zero is judged after reduction"""
    x %= L
    return (pow(x, -1, L), 1) if x else (0, 0)


def is_canonical(x):
    return int(x < L)


def _random(count, nbytes, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes(), "little") for _ in range(count)]


@functools.lru_cache(maxsize=None)
def values32(n_random=4096):
    """the 32-byte cases: the edges of the reduction (multiples of L and their neighbours up to 15 L, which is just below 2^256),
    of the 252- and 255-bit splits, of every 30-bit limb of the division steps, and seeded random values"""
    v = [0, 1, 2, L - 1, L, L + 1]
    for k in range(2, 16):
        v += [k * L - 1, k * L, k * L + 1]
    v += [2**252 - 1, 2**252, 2**255 - 19, 2**256 - 1]
    for j in range(1, 9):
        v += [2**(30 * j) - 1, 2**(30 * j), 2**(30 * j) + 1, L - 2**(30 * j)]
    v += [pow(2, -1, L), pow(3, -1, L), pow(2**30, -1, L)]
    v += _random(n_random, 32, 0x5CA1A7)
    assert all(0 <= x < 2**256 for x in v)
    return tuple(v)


@functools.lru_cache(maxsize=None)
def values64(n_random=1024):
    """the 64-byte cases of ScalarReduce: the edges of sc_reduce512's two folds and of the 512-bit range"""
    top = (2**512 - 1) // L * L
    v = [0, L << 256, 2**256 - 1, 2**256, 2**385, 2**387 - 1, 2**512 - 1, top - 1, top, top + 1]
    v += _random(n_random, 64, 0x5CA1A8)
    assert all(0 <= x < 2**512 for x in v)
    return tuple(v)


def to_rows(values, nbytes=32):
    return np.stack([np.frombuffer(int(x).to_bytes(nbytes, "little"), np.uint8) for x in values]).copy()


def from_rows(rows):
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


@functools.lru_cache(maxsize=None)
def case_set():
    """The shared operands and the model's answers, computed once and never written (the arrays are read-only): x is values32, y and
    z are seeded permutations of it (so every edge meets random partners and the edges meet each other somewhere), w is values64."""
    xs = list(values32())
    rng = np.random.default_rng(0x5CA1A9)
    ys = [xs[i] for i in rng.permutation(len(xs))]
    ys[:8] = [0, L, L - 1, 1, 2**256 - 1, L + 1, 0, 15 * L]     # ... and met on purpose: x = 0, 1, 2, L - 1, L, L + 1, 2 L - 1, 2 L
    zs = [xs[i] for i in rng.permutation(len(xs))]
    ws = list(values64())
    inv = [invert(x) for x in xs]
    out = dict(
        x=to_rows(xs), y=to_rows(ys), z=to_rows(zs), w=to_rows(ws, 64),
        reduce=to_rows([reduce(w) for w in ws]),
        add=to_rows([add(a, b) for a, b in zip(xs, ys)]),
        sub=to_rows([sub(a, b) for a, b in zip(xs, ys)]),
        mul=to_rows([mul(a, b) for a, b in zip(xs, ys)]),
        negate=to_rows([negate(a) for a in xs]),
        complement=to_rows([complement(a) for a in xs]),
        muladd=to_rows([muladd(a, b, c) for a, b, c in zip(xs, ys, zs)]),
        recip=to_rows([r for r, _ in inv]),
        ok=np.array([k for _, k in inv], np.int32),
        canonical=np.array([is_canonical(a) for a in xs], np.int32),
    )
    for a in out.values():
        a.setflags(write=False)
    return out


def cycled(a, n):
    """n rows of a, cycled to length"""
    return np.ascontiguousarray(a[np.arange(n) % len(a)])
