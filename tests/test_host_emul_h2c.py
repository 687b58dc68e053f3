"""CPU tests of the hashing calls' lane functions (curve25519_amd/csrc/h2c25519.cuh: what c25519_ExpandMessageXmd_*,
ed25519_MapToCurve_*, ed25519_HashToCurve_*, ed25519_EncodeToCurve_*, ristretto255_HashToGroup_* and ed25519_HashToScalar_* run on the
device, and the host's h2c_make_tail in front of them).  The device source is compiled by g++ against the C model of the gfx950
primitives (tests/host_emul/h2c.cpp, tests/host_emul/build.py's open_lib) and judged byte for byte against the big-integer model
of RFC 9380 / RFC 9497 (tests/h2c_model.py) on the case set the GPU tests share."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import h2c_model as model
import test_h2c_model as published
from vectors import P

vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
CALLS = {"hash_to_curve": 0, "encode_to_curve": 1, "hash_to_group": 2, "hash_to_scalar": 3}


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_h2c_expand": ([vp, vp, sz, vp, sz, sz, sz], None), "emul_h2c_map": ([vp, vp, sz], None),
                    "emul_h2c_call": ([ci, vp, vp, sz, vp, sz, sz], None), "emul_h2c_fe_from_be48": ([vp, vp, sz], None)},
                   "h2c.cpp", "libc25519_emul_h2c.so")
    yield lib
    assert_no_mad_overflow(lib)


def call(lib, name, dst, msgs):
    n, size = msgs.shape
    out, before = np.full((n, 32), 0xA5, np.uint8), msgs.copy()
    lib.emul_h2c_call(CALLS[name], out.ctypes.data, msgs.ctypes.data, size, dst, len(dst), n)
    assert np.array_equal(msgs, before), "the messages are not written"
    return out


def one(lib, name, msg: bytes, dst: bytes) -> str:
    return call(lib, name, dst, np.frombuffer(msg, np.uint8).reshape(1, len(msg)))[0].tobytes().hex()


def test_expand_message_xmd_matches_the_model(lib):
    for dst, size, msgs, n_bytes in model.xmd_cases():
        out, before = np.full((len(msgs), n_bytes), 0xA5, np.uint8), msgs.copy()
        lib.emul_h2c_expand(out.ctypes.data, msgs.ctypes.data, size, dst, len(dst), n_bytes, len(msgs))
        assert np.array_equal(out, model.expected("xmd", dst, msgs, n_bytes)), (len(dst), size, n_bytes)
        assert np.array_equal(msgs, before)
    for msg, want in ((b"", "6b9a7312411d92f921c6f68ca0b6380730a1a4d982c507211a90964c394179ba"),
                      (b"abc", "0da749f12fbe5483eb066a5f595055679b976e93abe9be6f0f6318bce7aca8dc")):
        out = np.zeros(32, np.uint8)
        lib.emul_h2c_expand(out.ctypes.data, msg, len(msg), published.XMD_DST, len(published.XMD_DST), 32, 1)
        assert out.tobytes().hex() == want, "RFC 9380 K.3"


@pytest.mark.parametrize("name", sorted(CALLS))
def test_call_matches_the_model_on_the_case_set(lib, name):
    for dst, size, msgs in model.case_set():
        got, want = call(lib, name, dst, msgs), model.expected(name, dst, msgs)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert not len(bad), (name, len(dst), size, [(i, got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:2])
    assert_no_mad_overflow(lib)


def test_map_to_curve_matches_the_model(lib):
    u = model.map_inputs()
    got, before = np.full((len(u), 32), 0xA5, np.uint8), u.copy()
    lib.emul_h2c_map(got.ctypes.data, u.ctypes.data, len(u))
    assert np.array_equal(u, before)
    want = model.expected_map()
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), [(i, u[i].tobytes().hex(), got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:4]
    identity = "01" + "00" * 31
    assert got[0].tobytes().hex() == identity and got[4].tobytes().hex() == identity, "u = 0 and u = p give the identity"
    assert_no_mad_overflow(lib)


def test_the_published_vectors(lib):
    for msg, (x, y) in published.RO_POINTS.items():
        want = (int(y, 16) | (int(x, 16) & 1) << 255).to_bytes(32, "little").hex()
        assert one(lib, "hash_to_curve", msg, published.RO_DST) == want, msg
    assert one(lib, "hash_to_curve", b"", published.RO_DST) == "21dc15e10253796df23a7699c8a383ea624cce88c52431f6be220b1a56c8a609"
    for msg, (x, y) in published.NU_POINTS.items():
        want = (int(y, 16) | (int(x, 16) & 1) << 255).to_bytes(32, "little").hex()
        assert one(lib, "encode_to_curve", msg, published.NU_DST) == want, msg
    ctx = model.oprf_context_string()
    assert one(lib, "hash_to_group", published.OPRF_INPUT, b"HashToGroup-" + ctx) == published.OPRF_ELEMENT
    derive = published.OPRF_SEED + len(published.OPRF_INFO).to_bytes(2, "big") + published.OPRF_INFO + b"\x00"
    assert one(lib, "hash_to_scalar", derive, b"DeriveKeyPair" + ctx) == published.OPRF_SKS


def test_the_48_byte_reduction_at_its_edges(lib):
    """every limb pattern the fold can meet: zeros, ones, p and its neighbours under each of the 2^128 multiples, and seeded values"""
    rng = np.random.default_rng(0x48)
    vals = [0, 1, P - 1, P, P + 1, 2**255 - 1, 2**255, 2**256 - 1, 2**256, 2**384 - 1, 2**383, (2**128 - 1) << 256,
            (2**128 - 1) << 256 | P, 2**384 - 2**256 + P - 1, 38 * (2**128 - 1) + 2**255 - 20]
    vals += [int.from_bytes(rng.integers(0, 256, 48, dtype=np.uint8).tobytes(), "big") for _ in range(48)]
    rows = np.stack([np.frombuffer(v.to_bytes(48, "big"), np.uint8) for v in vals])
    out = np.full((len(vals), 32), 0xA5, np.uint8)
    lib.emul_h2c_fe_from_be48(out.ctypes.data, rows.ctypes.data, len(vals))
    for v, row in zip(vals, out):
        assert int.from_bytes(row.tobytes(), "little") == v % P, hex(v)
    assert_no_mad_overflow(lib)
