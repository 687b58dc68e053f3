"""CPU tests of the group calls' lane functions (curve25519_amd/csrc/ed_group.cuh: what ed25519_ScalarMult[_noclamp]_*,
ed25519_ScalarMultBase[_noclamp]_*, ed25519_PointAdd_* and ed25519_PointSub_* run on the device).  The device source is compiled by
g++ against the C model of the gfx950 primitives (tests/host_emul/group_ops.cpp, tests/host_emul/build.py's open_lib) and judged
against the big-integer model of the stated rule (tests/group_model.py) on the case set the GPU tests share."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import group_model as model
import key_model
from vectors import ED_B, L, ed_enc, ed_mul

vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
NEUTRAL_ENC = (1).to_bytes(32, "little")


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_group_scalarmult": ([vp, vp, vp, vp, sz, ci, ci], None), "emul_group_base": ([vp, vp, sz, ci], None),
                    "emul_group_add": ([vp, vp, vp, vp, sz, ci], None), "emul_group_digits": ([vp, vp, ci, ci], None)},
                   "group_ops.cpp", "libc25519_emul_group_ops.so")
    yield lib
    assert_no_mad_overflow(lib)


@pytest.fixture(scope="module")
def cases():
    return model.case_set()


def scalarmult(lib, sc, pt, w, clamp):
    n = len(sc)
    q, ok = np.full((n, 32), 0xA5, np.uint8), np.full(n, 7, np.int32)
    before = sc.copy()
    lib.emul_group_scalarmult(q.ctypes.data, ok.ctypes.data, sc.ctypes.data, pt.ctypes.data, n, w, int(clamp))
    assert np.array_equal(sc, before), "the scalar bytes are not written"
    return q, ok


@pytest.mark.parametrize("clamp", (True, False), ids=("clamped", "noclamp"))
@pytest.mark.parametrize("w", model.WINDOWS)
def test_scalarmult_matches_the_model(lib, cases, w, clamp):
    sc, pt, labels = cases
    want, want_ok = model.expected_scalarmult(sc, pt, clamp)
    got, got_ok = scalarmult(lib, sc, pt, w, clamp)
    assert np.array_equal(got_ok, want_ok), [(i, labels[i]) for i in np.flatnonzero(got_ok != want_ok)][:8]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, labels[i], sc[i].tobytes().hex(), got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:4]
    assert not got[want_ok == 0].any(), "a point that does not decode gives 32 zero bytes"
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("w", model.WINDOWS)
def test_digits_are_the_models(lib, w):
    n = model.DIGITS[w]
    for s in model.scalars():
        for clamp in (True, False):
            out = np.full(n, 99, np.int32)
            lib.emul_group_digits(out.ctypes.data, np.frombuffer(s, np.uint8).ctypes.data, w, int(clamp))
            assert list(out) == model.recode(model.scalar_value(s, clamp), w), (s.hex(), clamp)


@pytest.mark.parametrize("clamp", (True, False), ids=("clamped", "noclamp"))
def test_base_matches_the_model(lib, clamp):
    sc = np.stack([np.frombuffer(s, np.uint8) for s in model.scalars(n_random=24)])
    got = np.full((len(sc), 32), 0xA5, np.uint8)
    lib.emul_group_base(got.ctypes.data, sc.ctypes.data, len(sc), int(clamp))
    want = model.expected_base(sc, clamp)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, sc[i].tobytes().hex()) for i in bad][:4]
    if not clamp:
        assert got[0].tobytes() == NEUTRAL_ENC and got[6].tobytes() == NEUTRAL_ENC, "[0]B and [L]B"
    for w in model.WINDOWS:                                  # ... and the variable-base walk on enc(B) gives the same bytes
        base = np.tile(np.frombuffer(model.BASE, np.uint8), (len(sc), 1))
        q, ok = scalarmult(lib, sc, base, w, clamp)
        assert ok.all() and np.array_equal(q, want), w
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("sub", (False, True), ids=("add", "sub"))
def test_add_and_sub_match_the_model(lib, sub):
    p, q, names = model.add_cases()
    want, want_ok = model.expected_add(p, q, sub)
    n = len(p)
    got, got_ok = np.full((n, 32), 0xA5, np.uint8), np.full(n, 7, np.int32)
    lib.emul_group_add(got.ctypes.data, got_ok.ctypes.data, p.ctypes.data, q.ctypes.data, n, int(sub))
    assert np.array_equal(got_ok, want_ok), [(i, names[i]) for i in np.flatnonzero(got_ok != want_ok)][:8]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, names[i], got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:4]
    assert not got[want_ok == 0].any() and 0 < want_ok.sum() < n
    assert_no_mad_overflow(lib)


def test_add_laws(lib, cases):
    """P + (-P) and P - P are the neutral encoding, P + P is [2]P of the walk, and torsion + torsion stays in the torsion"""
    p, q, names = model.add_cases()
    n = len(p)

    def add(a, b, sub):
        r, ok = np.full((len(a), 32), 0xA5, np.uint8), np.full(len(a), 7, np.int32)
        lib.emul_group_add(r.ctypes.data, ok.ctypes.data, a.ctypes.data, b.ctypes.data, len(a), int(sub))
        return r, ok

    r, ok = add(p, q, False)
    neg = np.array([s.endswith("P + (-P)") for s in names])
    assert (ok[neg] == 1).sum() > 80 and all(x.tobytes() == NEUTRAL_ENC for x in r[neg & (ok == 1)])
    r, ok = add(p, p, True)
    assert all(x.tobytes() == NEUTRAL_ENC for x in r[ok == 1]) and not r[ok == 0].any()
    dbl = np.array([s.endswith("P + P") for s in names])
    two = np.tile(np.frombuffer((2).to_bytes(32, "little"), np.uint8), (int(dbl.sum()), 1))
    r2, ok2 = add(p[dbl], q[dbl], False)
    for w in model.WINDOWS:
        m, mok = scalarmult(lib, two, p[dbl], w, False)
        assert np.array_equal(mok, ok2) and np.array_equal(m, r2), w
    tor = np.array([s == "torsion / torsion" for s in names])
    r, ok = add(p[tor], q[tor], False)
    small = {e for e in (x.tobytes() for x in r)}
    assert ok.all() and len(small) == 8, "the eight torsion points, canonically encoded"
    for e in small:
        assert key_model.classify(e) & key_model.SMALL_ORDER
    assert_no_mad_overflow(lib)


def test_known_multiples(lib):
    """[L - 1]B = -B, [L + 1]B = B, and a mixed-order point under 8: the torsion part is gone"""
    sc = np.stack([np.frombuffer(int(v).to_bytes(32, "little"), np.uint8) for v in (L - 1, L + 1, 8)])
    T8 = key_model.mixed_order_keys(np.frombuffer(model.BASE, np.uint8).reshape(1, 32))[0]
    pt = np.stack([np.frombuffer(b, np.uint8) for b in (model.BASE, model.BASE, T8)])
    minus_b = model.BASE[:31] + bytes([model.BASE[31] ^ 0x80])
    for w in model.WINDOWS:
        q, ok = scalarmult(lib, sc, pt, w, False)
        assert ok.all() and q[0].tobytes() == minus_b and q[1].tobytes() == model.BASE
        assert q[2].tobytes() == ed_enc(ed_mul(8, ED_B))
