"""CPU tests of the key calls' lane functions (curve25519_amd/csrc/ed_keys.cuh: what ed25519_ClassifyKey_*,
ed25519_PublicKey_to_X25519_* and ed25519_PrivateKey_to_X25519_* run on the device).  The device source is compiled by g++ against
the C model of the gfx950 primitives (tests/host_emul/key_convert.cpp, tests/host_emul/build.py's open_lib) and judged against the
big-integer model of the stated rule (tests/key_model.py) on the case set the GPU tests share."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import key_model as model
from vectors import L

vp, sz = C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_key_naf_masks": ([vp, vp], None), "emul_key_classify": ([vp, vp, sz], None),
                    "emul_key_to_x25519": ([vp, vp, vp, sz], None), "emul_key_private_to_x25519": ([vp, vp, sz], None),
                    "emul_key_order_parts": ([vp, vp, vp, vp, vp, sz], None)},
                   "key_convert.cpp", "libc25519_emul_key_convert.so")
    yield lib
    assert_no_mad_overflow(lib)


@pytest.fixture(scope="module")
def cases():
    keys, labels = model.case_set()
    return keys, labels, model.expected(keys)


def test_case_set_covers_every_class(cases):
    keys, labels, (flags, _, ok) = cases
    by = {lab: {int(f) for f, l in zip(flags, labels) if l == lab} for lab in set(labels)}
    assert by["honest"] == {11} and by["honest negated"] == {11}
    assert by["mixed order"] == {3}, "decodes, canonical, not small, NOT torsion-free"
    assert len([l for l in labels if l == "small order"]) == 14 and all(f & 4 for f in by["small order"])
    assert by["off the curve"] <= {0, 2}
    assert 0 < ok.sum() < len(ok)


def test_flags_match_the_model(lib, cases):
    keys, labels, (flags, _, _) = cases
    got = np.full(len(keys), 0xA5A5A5A5, np.uint32)
    lib.emul_key_classify(got.ctypes.data, keys.ctypes.data, len(keys))
    bad = [(i, labels[i], keys[i].tobytes().hex(), int(got[i]), int(flags[i])) for i in np.flatnonzero(got != flags)]
    assert not bad, bad[:8]
    assert not (got[(got & 1) == 0] & 12).any(), "bits 2 and 3 are clear where bit 0 is"
    assert_no_mad_overflow(lib)


def test_conversion_matches_the_model(lib, cases):
    keys, labels, (flags, xpk, ok) = cases
    got = np.full((len(keys), 32), 0xA5, np.uint8)
    got_ok = np.full(len(keys), 7, np.int32)
    lib.emul_key_to_x25519(got.ctypes.data, got_ok.ctypes.data, keys.ctypes.data, len(keys))
    assert np.array_equal(got_ok, ok), [(i, labels[i]) for i in np.flatnonzero(got_ok != ok)][:8]
    assert np.array_equal(got_ok, ((flags & 13) == 9).astype(np.int32))
    bad = np.flatnonzero((got != xpk).any(axis=1))
    assert not len(bad), [(i, labels[i], got[i].tobytes().hex(), xpk[i].tobytes().hex()) for i in bad][:4]
    assert not got[ok == 0].any(), "a rejected key's row is 32 zero bytes"
    assert not (got[:, 31] & 0x80).any(), "bit 255 is clear"
    assert_no_mad_overflow(lib)


def test_private_key_is_the_clamped_hash_of_the_seed_half(lib):
    rng = np.random.default_rng(0x5EED)
    priv = rng.integers(0, 256, (40, 64), dtype=np.uint8)
    priv[0] = 0
    priv[1] = 0xFF
    priv[2, 32:] = priv[3, 32:]                  # the second half is ignored
    priv[3, :32] = priv[2, :32]
    got = np.full((len(priv), 32), 0xA5, np.uint8)
    lib.emul_key_private_to_x25519(got.ctypes.data, priv.ctypes.data, len(priv))
    for i in range(len(priv)):
        d = bytearray(hashlib.sha512(priv[i, :32].tobytes()).digest()[:32])
        d[0] &= 248
        d[31] &= 127
        d[31] |= 64
        assert got[i].tobytes() == bytes(d) == model.private_to_x25519(priv[i].tobytes()), i
    assert np.array_equal(got[2], got[3])


def test_digit_masks_of_L(lib):
    """the generated masks sum back to L, no two non-zero digits are adjacent, a sign bit only sits on a non-zero digit, the top
    digit is +1 at bit 252 and every other one lies below bit 126"""
    nzw, ngw = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    lib.emul_key_naf_masks(nzw.ctypes.data, ngw.ctypes.data)
    nz = int.from_bytes(nzw.tobytes(), "little")
    neg = int.from_bytes(ngw.tobytes(), "little")
    assert sum((-1 if (neg >> i) & 1 else 1) << i for i in range(256) if (nz >> i) & 1) == L
    assert nz & (nz >> 1) == 0
    assert neg & ~nz == 0
    assert nz >> 252 == 1 and not (neg >> 252) & 1
    assert (nz & ((1 << 252) - 1)) < 1 << 126
    assert bin(nz).count("1") <= 47


def test_small_order_predicate_is_times_eight_and_the_walk_is_times_L(lib, cases):
    """on every decodable case: the byte predicate behind SMALL_ORDER equals [8]A = O computed by the lane's own doublings, and the
    walk's point is [L]A of the model (a torsion point for the mixed-order keys, not just 'something that is not O')"""
    keys, labels, (flags, _, _) = cases
    n = len(keys)
    dec, small, t8 = (np.full(n, 7, np.int32) for _ in range(3))
    xy = np.zeros((n, 64), np.uint8)
    lib.emul_key_order_parts(dec.ctypes.data, small.ctypes.data, t8.ctypes.data, xy.ctypes.data, keys.ctypes.data, n)
    assert np.array_equal(dec, (flags & 1).astype(np.int32))
    on = dec == 1
    assert on.sum() > 100
    assert np.array_equal(small[on], t8[on]), [labels[i] for i in np.flatnonzero(on & (small != t8))]
    assert np.array_equal(small[on], ((flags[on] & 4) != 0).astype(np.int32))
    seen = set()
    for i in np.flatnonzero(on):
        want = model.times_L(keys[i].tobytes())
        got = (int.from_bytes(xy[i, :32].tobytes(), "little"), int.from_bytes(xy[i, 32:].tobytes(), "little"))
        assert got == want, (i, labels[i])
        seen.add(want)
    assert len(seen) == 8, "the walk lands on every one of the eight torsion points"
    assert_no_mad_overflow(lib)
