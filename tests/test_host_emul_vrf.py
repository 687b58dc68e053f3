"""CPU tests of the ECVRF calls' lane functions (curve25519_amd/csrc/vrf25519.cuh: what ed25519_VRF_Prove_*, ed25519_VRF_Verify_* and
ed25519_VRF_ProofToHash_* run on the device, and the host's vrf_make_tail in front of them).  The device source is compiled by g++
against the C model of the gfx950 primitives (tests/host_emul/vrf.cpp, tests/host_emul/build.py's open_lib) and judged byte for
byte against the big-integer model of RFC 9381 (tests/vrf_model.py) on the case set the GPU tests share and on the RFC's three
examples."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import vrf_model as model

vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_vrf_prove": ([vp, vp, vp, sz, sz], None), "emul_vrf_verify": ([vp, vp, vp, vp, vp, sz, sz], None),
                    "emul_vrf_proof_to_hash": ([vp, vp, vp, sz], None), "emul_vrf_digits": ([vp, vp, ci], None)},
                   "vrf.cpp", "libc25519_emul_vrf.so")
    yield lib
    assert_no_mad_overflow(lib)


def prove(lib, priv, alpha):
    n = len(priv)
    out, before = np.full((n, 80), 0xA5, np.uint8), (priv.copy(), alpha.copy())
    lib.emul_vrf_prove(out.ctypes.data, np.ascontiguousarray(priv).ctypes.data, np.ascontiguousarray(alpha).ctypes.data, alpha.shape[1], n)
    assert np.array_equal(priv, before[0]) and np.array_equal(alpha, before[1])
    return out


def verify(lib, pk, pi, alpha):
    n = len(pk)
    beta, ok = np.full((n, 64), 0xA5, np.uint8), np.full(n, -1, np.int32)
    lib.emul_vrf_verify(beta.ctypes.data, ok.ctypes.data, np.ascontiguousarray(pk).ctypes.data, np.ascontiguousarray(pi).ctypes.data,
                        np.ascontiguousarray(alpha).ctypes.data, alpha.shape[1], n)
    return beta, ok


def proof_to_hash(lib, pi):
    n = len(pi)
    beta, ok = np.full((n, 64), 0xA5, np.uint8), np.full(n, -1, np.int32)
    lib.emul_vrf_proof_to_hash(beta.ctypes.data, ok.ctypes.data, np.ascontiguousarray(pi).ctypes.data, n)
    return beta, ok


@pytest.mark.parametrize("alpha_len", model.ALPHA_LENGTHS)
def test_honest_rows_match_the_model(lib, alpha_len):
    h = model.honest(alpha_len)
    assert np.array_equal(prove(lib, h["priv"], h["alpha"]), h["pi"])
    beta, ok = verify(lib, h["pk"], h["pi"], h["alpha"])
    assert ok.tolist() == [1] * len(ok) and np.array_equal(beta, h["beta"])
    beta, ok = proof_to_hash(lib, h["pi"])
    assert ok.tolist() == [1] * len(ok) and np.array_equal(beta, h["beta"])


def test_rejection_rows_match_the_model(lib):
    r = model.rejections()
    beta, ok = verify(lib, r["pk"], r["pi"], r["alpha"])
    bad = [lab for lab, g, w in zip(r["labels"], ok, r["ok"]) if g != w]
    assert not bad, bad
    assert np.array_equal(beta, r["beta"])
    beta, ok = proof_to_hash(lib, r["pi"])
    bad = [lab for lab, g, w in zip(r["labels"], ok, r["ok_hash"]) if g != w]
    assert not bad, bad
    assert np.array_equal(beta, r["beta_hash"])


def test_the_public_half_is_read_as_given(lib):
    priv, alpha, pi = model.mixed_order_privs()
    assert np.array_equal(prove(lib, priv, alpha), pi)


def test_the_published_examples(lib):
    for priv, pk, alpha, pi, beta in model.example_rows():
        a = np.frombuffer(alpha, np.uint8).reshape(1, len(alpha))
        got = prove(lib, np.frombuffer(priv, np.uint8).reshape(1, 64), a)
        assert got.tobytes().hex() == pi.hex()
        b, ok = verify(lib, np.frombuffer(pk, np.uint8).reshape(1, 32), got, a)
        assert ok.tolist() == [1] and b.tobytes().hex() == beta.hex()
        b, ok = proof_to_hash(lib, got)
        assert ok.tolist() == [1] and b.tobytes().hex() == beta.hex()


def test_the_recoding_at_both_lengths(lib):
    """the two-bit signed digits sum back to the scalar and stay in [-2, 1], at 129 digits below 2^255 and 65 below 2^128"""
    rng = np.random.default_rng(0x9381)
    for full, bits, digits in ((1, 255, 129), (0, 128, 65)):
        vals = [0, 1, 2, 3, 2**bits - 1, 2**(bits - 1), (2**bits - 1) // 3, 2 * (2**bits - 1) // 3]
        vals += [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % 2**bits for _ in range(24)]
        for v in vals:
            out = np.zeros(digits, np.int32)
            lib.emul_vrf_digits(out.ctypes.data, v.to_bytes(32, "little"), full)
            assert out.min() >= -2 and out.max() <= 1, hex(v)
            assert sum(int(d) << (2 * i) for i, d in enumerate(out)) == v, hex(v)
