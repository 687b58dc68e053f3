"""CPU tests of the scalar calls' lane functions (curve25519_amd/csrc/sc_invert.cuh: what ed25519_ScalarReduce_*, _ScalarAdd_*,
_ScalarSub_*, _ScalarMul_*, _ScalarNegate_*, _ScalarComplement_*, _ScalarMulAdd_*, _ScalarInvert_* and _ScalarIsCanonical_* run on the
device).  The device source is compiled by g++ against the C model of the gfx950 primitives (tests/host_emul/scalar.cpp,
tests/host_emul/build.py's open_lib) and judged byte for byte against the big-integer model (tests/scalar_model.py) on the case set
the GPU tests share; the model's overflow counter watches every signed multiply-add of the division steps mod L."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import scalar_model as model
from scalar_model import KS, L

vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
OPS = {"reduce": 0, "add": 1, "sub": 2, "mul": 3, "negate": 4, "complement": 5, "muladd": 6}      # sc_invert.cuh: ScOp
INPUTS = {"reduce": ("w",), "add": ("x", "y"), "sub": ("x", "y"), "mul": ("x", "y"), "negate": ("x",), "complement": ("x",),
          "muladd": ("x", "y", "z")}
FILL = 0xA5


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_scalar_op": ([ci, vp, vp, vp, vp, sz], None), "emul_scalar_is_canonical": ([vp, vp, sz], None),
                    "emul_scalar_invert": [vp, vp, vp, sz, ci], "emul_scalar_invert_words": ([vp, vp, sz], None)},
                   "scalar.cpp", "libc25519_emul_scalar.so")
    yield lib
    assert_no_mad_overflow(lib)


@pytest.fixture(scope="module")
def cases():
    return model.case_set()


def run_op(lib, name, inputs, out=None):
    """the call on copies of the inputs (out: one of the copies, for the in-place form); returns (result, the copies)"""
    ins = [a.copy() for a in inputs]
    n = len(ins[0])
    r = np.full((n, 32), FILL, np.uint8) if out is None else ins[out]
    ptrs = [a.ctypes.data for a in ins] + [None] * (3 - len(ins))
    lib.emul_scalar_op(OPS[name], r.ctypes.data, *ptrs, n)
    return r, ins


def invert(lib, s, k, in_place=False):
    s = s.copy()
    n = len(s)
    recip = s if in_place else np.full((n, 32), FILL, np.uint8)
    ok = np.full(n, 7, np.int32)
    assert lib.emul_scalar_invert(recip.ctypes.data, ok.ctypes.data, s.ctypes.data, n, k) == k
    return recip, ok, s


def rows_differ(got, want):
    return np.flatnonzero((got != want).any(axis=1))


@pytest.mark.parametrize("name", sorted(OPS))
def test_elementwise_call_matches_the_model(lib, cases, name):
    inputs = [cases[k] for k in INPUTS[name]]
    got, after = run_op(lib, name, inputs)
    bad = rows_differ(got, cases[name])
    assert not len(bad), [(int(i), [a[i].tobytes().hex() for a in inputs], got[i].tobytes().hex(), cases[name][i].tobytes().hex()) for i in bad][:4]
    assert all(np.array_equal(a, b) for a, b in zip(after, inputs)), "inputs are never written"
    assert all(v < L for v in model.from_rows(got[:128])), "every output is canonical"
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("name", sorted(set(OPS) - {"reduce"}))
def test_elementwise_call_in_place(lib, cases, name):
    """the output buffer may be exactly one of the input buffers (ScalarReduce's input rows are 64 bytes: no output buffer is its input)"""
    inputs = [cases[k] for k in INPUTS[name]]
    for which in range(len(inputs)):
        got, after = run_op(lib, name, inputs, out=which)
        assert not len(rows_differ(got, cases[name])), (name, which)
        assert all(np.array_equal(a, b) for j, (a, b) in enumerate(zip(after, inputs)) if j != which)


def test_is_canonical_matches_the_model(lib, cases):
    x = cases["x"].copy()
    ok = np.full(len(x), 7, np.int32)
    lib.emul_scalar_is_canonical(ok.ctypes.data, x.ctypes.data, len(x))
    assert np.array_equal(ok, cases["canonical"]) and np.array_equal(x, cases["x"])


def test_invert_words_on_the_whole_case_set(lib, cases):
    """sc_invert_words alone: every case, zeros and multiples of L included (0 -> 0), without the zero swap in front of it"""
    x = cases["x"].copy()
    got = np.full((len(x), 32), FILL, np.uint8)
    lib.emul_scalar_invert_words(got.ctypes.data, x.ctypes.data, len(x))
    bad = rows_differ(got, cases["recip"])
    assert not len(bad), [(int(i), x[i].tobytes().hex(), got[i].tobytes().hex(), cases["recip"][i].tobytes().hex()) for i in bad][:4]
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("k", KS)
def test_invert_matches_the_model_on_the_whole_case_set(lib, cases, k):
    recip, ok, after = invert(lib, cases["x"], k)
    assert np.array_equal(ok, cases["ok"]), np.flatnonzero(ok != cases["ok"])[:8]
    bad = rows_differ(recip, cases["recip"])
    assert not len(bad), [(int(i), cases["x"][i].tobytes().hex(), recip[i].tobytes().hex(), cases["recip"][i].tobytes().hex()) for i in bad][:4]
    assert np.array_equal(after, cases["x"]), "inputs are never written"
    assert not recip[cases["ok"] == 0].any(), "a zero's output is 32 zero bytes"
    in_place, ok2, _ = invert(lib, cases["x"], k, in_place=True)
    assert np.array_equal(in_place, cases["recip"]) and np.array_equal(ok2, cases["ok"]), "recip may be s itself"
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("k", KS)
def test_invert_at_the_group_edges(lib, cases, k):
    """n = 1, K - 1, K, K + 1, 3 K + 1: whole groups, a ragged tail of every kind, one lane and several; rows from the middle of the case
    set (random values) and from its head (the edges), and nothing is written past row n"""
    for n in sorted({1, k - 1, k, k + 1, 3 * k + 1} - {0}):
        for start in (0, 200):
            s = cases["x"][start:start + n]
            pad = np.full((n + 2, 32), FILL, np.uint8)
            okp = np.full(n + 2, 7, np.int32)
            sc = s.copy()
            assert lib.emul_scalar_invert(pad.ctypes.data, okp.ctypes.data, sc.ctypes.data, n, k) == k
            assert np.array_equal(pad[:n], cases["recip"][start:start + n]), (k, n, start)
            assert np.array_equal(okp[:n], cases["ok"][start:start + n]), (k, n, start)
            assert (pad[n:] == FILL).all() and (okp[n:] == 7).all(), "rows past n are not written"


@pytest.mark.parametrize("k", KS)
def test_invert_with_zeros_in_the_group(lib, k):
    """a zero (0, L, or 2 L: zero after reduction) in each single slot of a group, two zeros, and a group of zeros only: the zero's row
    is zero bytes with ok = 0 and every other row of the group is still its own inverse"""
    rng = np.random.default_rng(0x2E20 + k)
    vals = [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") for _ in range(3 * k)]
    assert all(v % L for v in vals)
    zeros = (0, L, 2 * L)
    patterns = [(j,) for j in range(k)] + ([(0, k - 1), (k // 2 - 1, k // 2)] if k > 1 else []) + [tuple(range(k))]
    for p, at in enumerate(patterns):
        v = list(vals)
        for j in at:
            v[k + j] = zeros[(p + j) % 3]                     # the middle group of three
        s = model.to_rows(v)
        want = [model.invert(x) for x in v]
        recip, ok, _ = invert(lib, s, k)
        assert np.array_equal(ok, np.array([o for _, o in want], np.int32)), (k, at)
        assert np.array_equal(recip, model.to_rows([r for r, _ in want])), (k, at)
        assert ok.sum() == 3 * k - len(at)
    assert_no_mad_overflow(lib)


def test_an_unknown_group_size_is_not_run(lib, cases):
    s = cases["x"][:4].copy()
    out, ok = np.full((4, 32), FILL, np.uint8), np.full(4, 7, np.int32)
    assert lib.emul_scalar_invert(out.ctypes.data, ok.ctypes.data, s.ctypes.data, 4, 3) == 0
    assert (out == FILL).all()
