"""CPU tests of the strict verification (curve25519_amd/csrc/strict25519.cuh and the Strict branches of the lattice path: what
ed25519_VerifySignature_strict_* runs on the device).  The device source is compiled by g++ against the C model of the gfx950
primitives (tests/host_emul/verify_strict.cpp, tests/host_emul/build.py's build_lib): the predicates on raw values, the lane chain
and the per-wave code as 192 lock-step lanes.  Expected verdicts: the strict rule in Python big integers (tests/strict_cases.py) on
top of the reference's verdict (the oracle's, or tests/golden/degenerate_verify.npz's)."""
import ctypes as C
import os

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import strict_cases as sc
from vectors import L, P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
vp, sz = C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_strict_predicates": [vp, vp, sz], "emul_strict_key": [vp, vp, sz],
                    **{f: ([vp, vp, vp, vp, vp, vp, sz, sz, C.c_int], None) for f in ("emul_strict_lane", "emul_strict_waves")}},
                   "verify_strict.cpp", "libc25519_emul_verify_strict.so")
    yield lib
    assert_no_mad_overflow(lib)


def ptr(a):
    return a.ctypes.data_as(vp)


def run(lib, which, sig, pk, msg, cap_bits=0):
    sig, pk, msg = (np.ascontiguousarray(a, np.uint8) for a in (sig, pk, msg))
    n = sig.shape[0]
    ok, listed, rej = (np.zeros(n, np.int32) for _ in range(3))
    fn = lib.emul_strict_lane if which == "lane" else lib.emul_strict_waves
    fn(ptr(ok), ptr(listed), ptr(rej), ptr(sig), ptr(pk), ptr(msg), msg.shape[1], n, cap_bits)
    return ok, listed, rej


@pytest.fixture(scope="module")
def edges(oracle):
    sig, pk, msg = sc.edge_cases(oracle)
    return sig, pk, msg, sc.strict_rule(sig, pk, oracle.ed25519_verify(sig, pk, msg))


def test_predicates_at_their_boundaries(lib):
    """S < L, small y, the key's rules 2-3 and the pair's rules 1 and 5 on L - 1 / L / L + 1, p - 1 / p / p + 1, every small y and its
    neighbours, with bit 255 clear and set"""
    v = sc.predicate_values()
    out = np.zeros((len(v), 4), np.int32)
    lib.emul_strict_predicates(ptr(out), ptr(v), len(v))
    for i in range(len(v)):
        x = int.from_bytes(v[i].tobytes(), "little")
        y = x & sc.MASK255
        small = y % P in sc.SMALL_Y
        want = [int(x < L), int(small), int(y >= P or small), int(x >= L or small)]
        assert list(out[i]) == want, hex(x)
    assert {L - 1, L}.issubset({int.from_bytes(r.tobytes(), "little") for r in v})


def test_lane_chain_equals_the_rule(lib, edges):
    sig, pk, msg, want = edges
    ok, listed, rej = run(lib, "lane", sig, pk, msg)
    assert np.array_equal(ok, want), np.nonzero(ok != want)[0][:10]
    assert not listed[rej == 1].any()
    assert want.sum() >= 16 and (want == 0).sum() > len(want) // 2                # both verdicts are exercised


def test_lane_chain_off_curve_keys_are_not_listed(lib, edges):
    """a key off the curve breaks rule 4: verdict 0 from the walk, nothing for the reference-order kernel"""
    sig, pk, msg, _ = edges
    off = np.array([sc.ed_decode(int.from_bytes(k.tobytes(), "little") & sc.MASK255, k[31] >> 7) is None for k in pk])
    assert off.sum() >= 12
    ok, listed, rej = run(lib, "lane", sig[off], pk[off], msg[off])
    assert not ok.any() and not listed.any() and rej.all()


def test_lane_chain_over_long_vectors_keep_strict_verdicts(lib, edges):
    """a low lattice cap sends honest elements to the reference order: they must still get the strict verdict"""
    sig, pk, msg, want = edges
    ok, listed, rej = run(lib, "lane", sig, pk, msg, cap_bits=100)
    assert listed.sum() > len(sig) // 4
    assert np.array_equal(ok, want)


def test_degenerate_golden_lane(lib):
    g = np.load(os.path.join(GOLD, "degenerate_verify.npz"))
    want = sc.strict_rule(g["sig"], g["pk"], g["verdict"])
    assert g["verdict"].sum() > want.sum()                                       # the set is where the two semantics differ
    ok, listed, rej = run(lib, "lane", g["sig"], g["pk"], g["msg"])
    assert np.array_equal(ok, want), np.nonzero(ok != want)[0][:10]
    assert not listed.any()


def test_wave_key_check_equals_rules_2_to_4(lib, edges):
    """coop::strict_key_ok, the per-workgroup key check of ed25519_Verify_Check_strict_*, on every distinct key of the edge set (small
    order in every encoding, y >= p with both sign bits, off the curve, mixed order, honest), all 64 lanes agreeing"""
    _, pk, _, _ = edges
    keys = np.unique(pk, axis=0)
    ok = np.zeros(len(keys), np.int32)
    lib.emul_strict_key(ptr(ok), ptr(np.ascontiguousarray(keys)), len(keys))
    want = []
    for k in keys:
        a = int.from_bytes(k.tobytes(), "little")
        y = a & sc.MASK255
        want.append(int(y < P and y % P not in sc.SMALL_Y and sc.ed_decode(y, a >> 255) is not None))
    assert list(ok) == want
    assert 0 < sum(want) < len(want) - 20


def _subset(sig, pk, msg, want, step):
    idx = np.arange(0, len(sig), step)
    return sig[idx], pk[idx], msg[idx], want[idx]


def test_three_waves_equal_the_rule(lib, edges):
    """coop::verify_three_waves<true>, one element per 192-lane workgroup; every element gets a verdict"""
    sig, pk, msg, want = _subset(*edges, 3)
    ok, listed, rej = run(lib, "waves", sig, pk, msg)
    assert np.array_equal(ok, want), np.nonzero(ok != want)[0][:10]
    assert not listed[rej == 1].any()
    assert want.sum() >= 4


def test_three_waves_degenerate_golden(lib):
    g = np.load(os.path.join(GOLD, "degenerate_verify.npz"))
    idx = np.concatenate([np.nonzero(g["verdict"] == 1)[0][::4], np.nonzero(g["label"] >= 3)[0][::5]])
    want = sc.strict_rule(g["sig"][idx], g["pk"][idx], g["verdict"][idx])
    ok, listed, rej = run(lib, "waves", g["sig"][idx], g["pk"][idx], g["msg"][idx])
    assert np.array_equal(ok, want)
    assert not listed.any()


def _libcrypto():
    for name in ("libcrypto.so.3",):
        try:
            return C.CDLL(name)
        except OSError:
            pass
    return None


def test_openssl_agrees_where_it_checks_the_same(edges):
    """second opinion: libcrypto's Ed25519 (EVP_DigestVerify) on the edge cases that keep rules 2, 3 and 5 -- where OpenSSL 3.0 and the
    strict rule coincide (it checks S < L and the key's decoding, not small order)"""
    lc = _libcrypto()
    if lc is None:
        pytest.skip("libcrypto.so.3 not loadable")
    lc.EVP_PKEY_new_raw_public_key.restype = vp
    lc.EVP_PKEY_new_raw_public_key.argtypes = [C.c_int, vp, C.c_char_p, sz]
    lc.EVP_MD_CTX_new.restype = vp
    lc.EVP_DigestVerifyInit.argtypes = [vp, vp, vp, vp, vp]
    lc.EVP_DigestVerify.argtypes = [vp, C.c_char_p, sz, C.c_char_p, sz]
    lc.EVP_MD_CTX_free.argtypes = [vp]
    lc.EVP_PKEY_free.argtypes = [vp]
    sig, pk, msg, want = edges
    checked = 0
    for i in range(len(sig)):
        a = int.from_bytes(pk[i].tobytes(), "little") & sc.MASK255
        yR = int.from_bytes(sig[i][:32].tobytes(), "little") & sc.MASK255
        if a >= P or a in sc.SMALL_Y or yR % P in sc.SMALL_Y:
            continue
        key = lc.EVP_PKEY_new_raw_public_key(1087, None, pk[i].tobytes(), 32)           # EVP_PKEY_ED25519
        got = 0
        if key:
            ctx = lc.EVP_MD_CTX_new()
            if lc.EVP_DigestVerifyInit(ctx, None, None, None, key) == 1:
                got = 1 if lc.EVP_DigestVerify(ctx, sig[i].tobytes(), 64, msg[i].tobytes(), msg.shape[1]) == 1 else 0
            lc.EVP_MD_CTX_free(ctx)
            lc.EVP_PKEY_free(key)
        assert got == want[i], i
        checked += 1
    assert checked > 100
