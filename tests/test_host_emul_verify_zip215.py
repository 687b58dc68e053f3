"""CPU tests of the ZIP-215 verification (what ed25519_VerifySignature_zip215_* runs on the device).  The device source is compiled by
g++ against the C model of the gfx950 primitives (tests/host_emul/verify_zip215.cpp, tests/host_emul/build.py's build_lib): the
decoding, the lane chain, the quad walk and the per-wave code as lock-step lanes, and the cofactored reference-order fallback.
Expected verdicts: the rule in Python big integers (tests/zip215_cases.py), whose own properties are asserted first."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import zip215_cases as zc
from vectors import L, P

vp, sz = C.c_void_p, C.c_size_t
SHAPES = ("lane", "quad", "waves")


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_zip215_decode": [vp, vp, vp, sz], "emul_zip215_plain_strict": [vp, vp, vp, vp, vp, sz, sz],
                    **{"emul_zip215_" + s: ([vp, vp, vp, vp, vp, vp, sz, sz, C.c_int], None) for s in SHAPES}},
                   "verify_zip215.cpp", "libc25519_emul_verify_zip215.so")
    yield lib
    assert_no_mad_overflow(lib)


def ptr(a):
    return a.ctypes.data_as(vp)


def run(lib, which, sig, pk, msg, cap_bits=0):
    sig, pk, msg = (np.ascontiguousarray(a, np.uint8) for a in (sig, pk, msg))
    n = sig.shape[0]
    ok, listed, rej = (np.zeros(n, np.int32) for _ in range(3))
    getattr(lib, "emul_zip215_" + which)(ptr(ok), ptr(listed), ptr(rej), ptr(sig), ptr(pk), ptr(msg), msg.shape[1], n, cap_bits)
    return ok, listed, rej


@pytest.fixture(scope="module")
def edges(oracle):
    sig, pk, msg = zc.edge_set(oracle)
    return sig, pk, msg, zc.zip215_rule(sig, pk, msg)


@pytest.fixture(scope="module")
def grid():
    sig, pk, msg = zc.conformance_grid()
    return sig, pk, msg


# ---- the model itself -----------------------------------------------------------------------------------------------------

def test_model_accepts_the_whole_conformance_grid(grid):
    sig, pk, msg = grid
    assert len(sig) == 196 and len(np.unique(pk, axis=0)) == 14
    assert zc.zip215_rule(sig, pk, msg).sum() == 196


def test_model_accepts_every_torsion_shifted_signature(oracle):
    sig, pk, msg = zc.torsion()
    assert len(sig) == 24 and zc.zip215_rule(sig, pk, msg).sum() == 24
    assert 0 < oracle.ed25519_verify(sig, pk, msg).sum() < 24                    # the plain rule: only j + h*t = 0 mod 8


def test_model_on_the_degenerate_set():
    sig, pk, msg, label = zc.degenerate()
    got = zc.zip215_rule(sig, pk, msg)
    assert len(sig) == 1024 and got.sum() == 388
    assert {int(k): (int(got[label == k].sum()), int((label == k).sum())) for k in np.unique(label)} == \
        {0: (124, 496), 1: (180, 180), 2: (0, 96), 3: (42, 126), 4: (42, 126)}
    S = np.array([int.from_bytes(s[32:].tobytes(), "little") for s in sig], dtype=object)
    assert not got[S >= L].any()                                                  # every S in {L, 2L, 15L, S + L}
    assert got[(S == 0)].all() and not got[S == 1].any()


def test_model_decodes_twelve_of_the_nineteen_non_canonical_y():
    ok = sorted({(int.from_bytes(r.tobytes(), "little") & zc.MASK255) - P for r in zc.noncanonical_y_strings()
                 if zc.zip215_decode(r) is not None})
    assert ok == [0, 1, 3, 4, 5, 6, 9, 10, 14, 15, 16, 18]
    for r in zc.noncanonical_y_strings():                                         # the sign bit never decides whether a string decodes
        flipped = r.copy()
        flipped[31] ^= 0x80
        assert (zc.zip215_decode(r) is None) == (zc.zip215_decode(flipped) is None)


def test_model_differs_from_plain_and_strict_on_the_edge_set(oracle, edges):
    import strict_cases as sc
    sig, pk, msg, want = edges
    plain = oracle.ed25519_verify(sig, pk, msg)
    strict = sc.strict_rule(sig, pk, plain)
    assert ((want == 1) & (plain == 0)).sum() >= 16 and ((want == 0) & (plain == 1)).sum() >= 16
    assert ((want == 1) & (strict == 0)).sum() >= 16 and not ((want == 0) & (strict == 1)).any()
    assert want.sum() >= 64 and (want == 0).sum() >= 64


# ---- (a) decoding ---------------------------------------------------------------------------------------------------------

def test_decode_equals_the_model(lib):
    enc = np.ascontiguousarray(zc.decode_inputs())
    assert len(enc) == 38 + 14 + 2
    xy = np.zeros((len(enc), 64), np.uint8)
    ok = np.zeros(len(enc), np.int32)
    lib.emul_zip215_decode(ptr(xy), ptr(ok), ptr(enc), len(enc))
    for i in range(len(enc)):
        pt = zc.zip215_decode(enc[i])
        assert ok[i] == int(pt is not None), i
        if pt is not None:
            got = (int.from_bytes(xy[i, :32].tobytes(), "little"), int.from_bytes(xy[i, 32:].tobytes(), "little"))
            assert got == pt, i
    assert ok[:38].sum() == 24 and ok[38:].all()


# ---- (b) the three shapes on the edge set ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_shape_equals_the_model_on_the_edge_set(lib, edges, shape):
    sig, pk, msg, want = edges
    if shape == "waves":                                                          # 192 lock-step lanes per element: every third one
        sig, pk, msg, want = (a[::3] for a in edges)
    ok, listed, rej = run(lib, shape, sig, pk, msg)
    assert np.array_equal(ok, want), np.nonzero(ok != want)[0][:10]
    assert not listed.any()                                                       # nothing is over-long at the default cap
    assert rej.sum() >= 8 and not ok[rej == 1].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_shape_accepts_the_conformance_grid(lib, grid, shape):
    sig, pk, msg = (a[::5] for a in grid) if shape == "waves" else grid
    ok, listed, rej = run(lib, shape, sig, pk, msg)
    assert ok.all() and not listed.any() and not rej.any()


@pytest.mark.parametrize("shape", ("lane", "quad"))
def test_shape_on_the_degenerate_and_torsion_sets(lib, shape):
    sig, pk, msg, _ = zc.degenerate()
    idx = np.arange(0, len(sig), 3)
    ok, listed, rej = run(lib, shape, sig[idx], pk[idx], msg[idx])
    assert np.array_equal(ok, zc.zip215_rule(sig[idx], pk[idx], msg[idx]))
    sig, pk, msg = zc.torsion()
    ok, listed, rej = run(lib, shape, sig, pk, msg)
    assert ok.all()


def test_keys_and_r_off_the_curve_are_rejected_and_not_listed(lib, edges):
    sig, pk, msg, want = edges
    off = np.array([zc.zip215_decode(k) is None or zc.zip215_decode(s[:32]) is None for k, s in zip(pk, sig)])
    key_off = np.array([zc.zip215_decode(k) is None for k in pk])
    assert key_off.sum() >= 12 and (off & ~key_off).sum() >= 7
    for shape in ("lane", "quad"):
        ok, listed, rej = run(lib, shape, sig[off], pk[off], msg[off], cap_bits=100)
        assert not ok.any()
        kl = key_off[off]
        assert rej[kl].all() and not listed[kl].any()                             # a key without a square root goes on no list


# ---- (c) the cofactored fallback ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_over_long_vectors_get_the_model_verdict_from_the_fallback(lib, edges, shape):
    sig, pk, msg, want = (a[::4] for a in edges) if shape == "waves" else edges
    ok, listed, rej = run(lib, shape, sig, pk, msg, cap_bits=100)
    assert listed.sum() > 0
    assert np.array_equal(ok[listed == 1], want[listed == 1])
    assert want[listed == 1].any() and not want[listed == 1].all()                # the fallback says yes and no
    assert np.array_equal(ok, want)


def test_fallback_accepts_what_the_byte_comparison_rejects(lib, grid):
    """the grid and the torsion cases at a 100-bit cap: listed elements are accepted although enc(T) differs from the R bytes"""
    tsig, tpk, tmsg = zc.torsion()
    sig = np.concatenate([grid[0], tsig])
    pk = np.concatenate([grid[1], tpk])
    msg = np.concatenate([np.pad(grid[2], ((0, 0), (0, 27))), tmsg])              # one message length per call
    want = zc.zip215_rule(sig, pk, msg)
    ok, listed, rej = run(lib, "lane", sig, pk, msg, cap_bits=100)
    assert np.array_equal(ok, want)
    assert listed[len(grid[0]):].sum() > 0 and want[len(grid[0]):].all()


# ---- (d) honest signatures ------------------------------------------------------------------------------------------------

def test_honest_signatures_all_three_rule_sets_agree(lib, oracle):
    n = 48
    sk = oracle.random_bytes((n, 32), 0x21521501)
    pub, priv = oracle.ed25519_keypair(sk)
    msg = oracle.random_bytes((n, 40), 0x21521502)
    sig = oracle.ed25519_sign(priv, msg)
    sig[1::4, 7] ^= 0x10                                                          # every fourth one corrupted in R ...
    msg[2::4, 3] ^= 0x01                                                          # ... or in the message
    sig, pub, msg = (np.ascontiguousarray(a) for a in (sig, pub, msg))
    plain, strict = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lib.emul_zip215_plain_strict(ptr(plain), ptr(strict), ptr(sig), ptr(pub), ptr(msg), msg.shape[1], n)
    want = oracle.ed25519_verify(sig, pub, msg)
    assert np.array_equal(plain, want) and np.array_equal(strict, want) and want.sum() == n // 2
    for shape in SHAPES:
        idx = np.arange(0, n, 3 if shape == "waves" else 1)
        ok, _, _ = run(lib, shape, sig[idx], pub[idx], msg[idx])
        assert np.array_equal(ok, want[idx]), shape
    assert np.array_equal(zc.zip215_rule(sig[:12], pub[:12], msg[:12]), want[:12])
