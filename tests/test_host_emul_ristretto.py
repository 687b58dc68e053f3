"""CPU tests of the ristretto255 calls' lane functions (curve25519_amd/csrc/ristretto255.cuh: what ristretto255_IsValidPoint_*,
ristretto255_FromHash_*, ristretto255_ScalarMult_*, ristretto255_ScalarMultBase_*, ristretto255_PointAdd_* and ristretto255_PointSub_*
run on the device).  The device source is compiled by g++ against the C model of the gfx950 primitives (tests/host_emul/ristretto.cpp,
tests/host_emul/build.py's open_lib) and judged byte for byte against the big-integer model of RFC 9496 (tests/ristretto_model.py)
on the case set the GPU tests share."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import ristretto_model as model
from vectors import L, P

vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_rist_is_valid": ([vp, vp, sz], None), "emul_rist_from_hash": ([vp, vp, sz], None),
                    "emul_rist_scalarmult": ([vp, vp, vp, vp, sz, ci], None), "emul_rist_base": ([vp, vp, sz], None),
                    "emul_rist_add": ([vp, vp, vp, vp, sz, ci], None), "emul_rist_decode_encode": ([vp, vp, vp, vp, sz], None),
                    "emul_rist_encode_affine": ([vp, vp, vp, sz, ci], None)},
                   "ristretto.cpp", "libc25519_emul_ristretto.so")
    yield lib
    assert_no_mad_overflow(lib)


@pytest.fixture(scope="module")
def cases():
    return model.case_set()


def scalarmult(lib, sc, pt, w):
    n = len(sc)
    q, ok = np.full((n, 32), 0xA5, np.uint8), np.full(n, 7, np.int32)
    before = sc.copy()
    lib.emul_rist_scalarmult(q.ctypes.data, ok.ctypes.data, sc.ctypes.data, pt.ctypes.data, n, w)
    assert np.array_equal(sc, before), "the scalar bytes are not written"
    return q, ok


def test_is_valid_point_matches_the_model(lib):
    pts, labels = model.points()
    ok = np.full(len(pts), 7, np.int32)
    lib.emul_rist_is_valid(ok.ctypes.data, pts.ctypes.data, len(pts))
    want = model.expected_valid(pts)
    assert np.array_equal(ok, want), [(i, labels[i]) for i in np.flatnonzero(ok != want)][:8]
    assert 16 <= want.sum() <= len(pts) - 16
    assert_no_mad_overflow(lib)


def test_from_hash_matches_the_model(lib):
    h = model.hashes()
    got = np.full((len(h), 32), 0xA5, np.uint8)
    before = h.copy()
    lib.emul_rist_from_hash(got.ctypes.data, h.ctypes.data, len(h))
    want = model.expected_from_hash(h)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, h[i].tobytes().hex(), got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:4]
    assert np.array_equal(h, before)
    assert not got[0].any(), "64 zero bytes map to the identity"
    assert got[2].tobytes().hex() == "3066f82a1a747d45120d1740f14358531a8f04bbffe6a819f86dfe50f44a0a46", "the RFC's vector"
    ok = np.full(len(h), 7, np.int32)
    lib.emul_rist_is_valid(ok.ctypes.data, got.ctypes.data, len(h))
    assert (ok == 1).all(), "every output decodes"
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("w", model.WINDOWS)
def test_scalarmult_matches_the_model(lib, cases, w):
    sc, pt, labels = cases
    want, want_ok = model.expected_scalarmult(sc, pt)
    got, got_ok = scalarmult(lib, sc, pt, w)
    assert np.array_equal(got_ok, want_ok), [(i, labels[i]) for i in np.flatnonzero(got_ok != want_ok)][:8]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, labels[i], sc[i].tobytes().hex(), got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:4]
    assert not got[want_ok == 0].any(), "a point that does not decode gives 32 zero bytes"
    assert 0 < want_ok.sum() < len(sc)
    assert_no_mad_overflow(lib)


def test_base_matches_the_model(lib):
    sc = np.stack([np.frombuffer(s, np.uint8) for s in model.scalars(n_random=24)])
    got = np.full((len(sc), 32), 0xA5, np.uint8)
    before = sc.copy()
    lib.emul_rist_base(got.ctypes.data, sc.ctypes.data, len(sc))
    assert np.array_equal(sc, before)
    want = model.expected_base(sc)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, sc[i].tobytes().hex()) for i in bad][:4]
    assert not got[0].any() and not got[6].any(), "[0]B and [L]B are the identity: zero bytes"
    assert got[1].tobytes() == model.BASE
    for w in model.WINDOWS:                                  # ... and the variable-base walk on enc(B) gives the same bytes
        base = np.tile(np.frombuffer(model.BASE, np.uint8), (len(sc), 1))
        q, ok = scalarmult(lib, sc, base, w)
        assert ok.all() and np.array_equal(q, want), w
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("sub", (False, True), ids=("add", "sub"))
def test_add_and_sub_match_the_model(lib, sub):
    p, q, names = model.add_cases()
    want, want_ok = model.expected_add(p, q, sub)
    n = len(p)
    got, got_ok = np.full((n, 32), 0xA5, np.uint8), np.full(n, 7, np.int32)
    lib.emul_rist_add(got.ctypes.data, got_ok.ctypes.data, p.ctypes.data, q.ctypes.data, n, int(sub))
    assert np.array_equal(got_ok, want_ok), [(i, names[i]) for i in np.flatnonzero(got_ok != want_ok)][:8]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, names[i], got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:4]
    assert not got[want_ok == 0].any() and 0 < want_ok.sum() < n
    if sub:
        same = np.array([s.endswith("P, P") for s in names])
        assert not got[same].any(), "P - P is the identity: zero bytes (with ok = 1 where P decodes)"
    assert_no_mad_overflow(lib)


def test_decode_gives_the_models_point_and_encode_takes_it_back(lib):
    pts, labels = model.points()
    n = len(pts)
    enc, xy, ok = np.full((n, 32), 0xA5, np.uint8), np.full((n, 64), 0xA5, np.uint8), np.full(n, 7, np.int32)
    lib.emul_rist_decode_encode(enc.ctypes.data, xy.ctypes.data, ok.ctypes.data, pts.ctypes.data, n)
    for i in range(n):
        A = model.decode(pts[i].tobytes())
        assert ok[i] == (A is not None), labels[i]
        if A is not None:
            got = (int.from_bytes(xy[i, :32].tobytes(), "little"), int.from_bytes(xy[i, 32:].tobytes(), "little"))
            assert got == A, labels[i]
            assert enc[i].tobytes() == pts[i].tobytes(), labels[i]
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("with_t", (1, 0), ids=("with T", "re-formed"))
def test_encode_on_every_representative_and_projective_scale(lib, with_t):
    """the four points of a coset, each under three projective factors, encode to the element's bytes: both rotation outcomes and
    both forms of the encoder (T given, T re-formed)"""
    from vectors import ed_add
    i4 = model.SQRT_M1
    e4 = [(0, 1), (0, P - 1), (i4, 0), (P - i4, 0)]
    pts, labels = model.points()
    valid = [p.tobytes() for p, l in zip(pts, labels) if l == "valid"][:20]
    rows, zs, want, rot = [], [], [], []
    for k, b in enumerate(valid):
        A = model.decode(b)
        for T in e4:
            Q = ed_add(A, T)
            for z in (1, 2**255 - 20, 0x1234567 + k * 2**200):
                rows.append(Q[0].to_bytes(32, "little") + Q[1].to_bytes(32, "little"))
                zs.append(z.to_bytes(32, "little"))
                want.append(b)
                rot.append(model.encode_rotates(Q))
    assert 16 <= sum(rot) <= len(rot) - 16
    xy = np.stack([np.frombuffer(r, np.uint8) for r in rows])
    z = np.stack([np.frombuffer(r, np.uint8) for r in zs])
    got = np.full((len(rows), 32), 0xA5, np.uint8)
    lib.emul_rist_encode_affine(got.ctypes.data, xy.ctypes.data, z.ctypes.data, len(rows), with_t)
    bad = [i for i in range(len(rows)) if got[i].tobytes() != want[i]]
    assert not bad, bad[:8]
    assert_no_mad_overflow(lib)


def test_known_multiples(lib):
    """[L]P is the identity for every valid P (no cofactor left), [L - 1]B = -B encodes differently from B, [L + 1]B = B"""
    pts, labels = model.points()
    valid = np.stack([p for p, l in zip(pts, labels) if l == "valid"][:12])
    el = np.tile(np.frombuffer(L.to_bytes(32, "little"), np.uint8), (len(valid), 1))
    for w in model.WINDOWS:
        q, ok = scalarmult(lib, el, valid, w)
        assert ok.all() and not q.any(), w
    sc = np.stack([np.frombuffer(int(v).to_bytes(32, "little"), np.uint8) for v in (L - 1, L + 1, 2**255 + 1)])
    base = np.tile(np.frombuffer(model.BASE, np.uint8), (3, 1))
    q, ok = scalarmult(lib, sc, base, 2)
    assert ok.all() and q[1].tobytes() == model.BASE and q[2].tobytes() == model.BASE, "bit 255 of the scalar is ignored"
    assert q[0].tobytes() == model.scalarmult_base((L - 1).to_bytes(32, "little")) != model.BASE
