"""The hashing calls at the drop-in boundary without a device: every call fails with an error code and a message (EngineError through
curve25519_amd.api), there is no CPU result behind them, and n == 0 returns 0 all the same.  Argument errors -- null pointers, a
dst_len of 0 or 256, a len_in_bytes of 0 or 16321 -- are refused with a message before any device is asked for.  With a GPU present
the first half does not apply and only the argument rules are checked here (tests/test_gpu_h2c.py holds the rest)."""
import numpy as np
import pytest

from curve25519_amd import _lib, api

MSG_CALLS = ("ed25519_HashToCurve", "ed25519_EncodeToCurve", "ristretto255_HashToGroup", "ed25519_HashToScalar")
DST = b"QUUX-V01-CS02-no-device"


def has_device():
    return _lib.load().c25519_amd_device_count() > 0


def test_without_a_device_every_call_raises():
    msg = np.ones((2, 5), np.uint8)
    if has_device():
        assert api.ed25519_HashToScalar(msg, DST).shape == (2, 32)
        return
    for name in MSG_CALLS:
        with pytest.raises(_lib.EngineError):
            getattr(api, name)(msg, DST)
        assert _lib.load().c25519_amd_last_error() != b""
    with pytest.raises(_lib.EngineError):
        api.c25519_ExpandMessageXmd(msg, DST, 48)
    with pytest.raises(_lib.EngineError):
        api.ed25519_MapToCurve(np.ones((2, 32), np.uint8))
    assert _lib.load().c25519_amd_last_error() != b""


def test_without_a_device_no_call_leaves_a_result():
    if has_device():
        return
    lib = _lib.load()
    out, msg = np.full((3, 64), 0xA5, np.uint8), np.ones((3, 8), np.uint8)
    o, m = out.ctypes.data, msg.ctypes.data
    for name in MSG_CALLS:
        assert getattr(lib, name + "_batch")(o, m, 8, DST, len(DST), 3) != 0, name
        assert getattr(lib, name + "_dev")(o, m, 8, DST, len(DST), 3, None) != 0, name
        assert getattr(lib, name + "_batch")(o, None, 0, DST, len(DST), 3) != 0, name
    assert lib.c25519_ExpandMessageXmd_batch(o, m, 8, DST, len(DST), 64, 3) != 0
    assert lib.c25519_ExpandMessageXmd_dev(o, m, 8, DST, len(DST), 64, 3, None) != 0
    assert lib.ed25519_MapToCurve_batch(o, m, 3) != 0 and lib.ed25519_MapToCurve_dev(o, m, 3, None) != 0
    assert (out == 0xA5).all(), "a failed call writes no result"


def test_a_call_of_nothing_returns_zero():
    lib = _lib.load()
    buf = np.full((1, 64), 0xA5, np.uint8)
    p = buf.ctypes.data
    for name in MSG_CALLS:
        assert getattr(lib, name + "_batch")(p, p, 8, DST, len(DST), 0) == 0, name
        assert getattr(lib, name + "_dev")(p, p, 8, DST, len(DST), 0, None) == 0, name
        assert getattr(lib, name + "_batch")(p, None, 0, DST, len(DST), 0) == 0, "msg may be NULL when msg_size is 0"
    assert lib.c25519_ExpandMessageXmd_batch(p, p, 8, DST, len(DST), 64, 0) == 0
    assert lib.c25519_ExpandMessageXmd_dev(p, p, 8, DST, len(DST), 64, 0, None) == 0
    assert lib.ed25519_MapToCurve_batch(p, p, 0) == 0 and lib.ed25519_MapToCurve_dev(p, p, 0, None) == 0
    assert (buf == 0xA5).all()
    for name in MSG_CALLS:
        assert getattr(api, name)(np.zeros((0, 7), np.uint8), DST).shape == (0, 32)
    assert api.c25519_ExpandMessageXmd(np.zeros((0, 7), np.uint8), DST, 100).shape == (0, 100)
    assert api.ed25519_MapToCurve(np.zeros((0, 32), np.uint8)).shape == (0, 32)


def test_a_null_pointer_is_an_argument_error():
    lib = _lib.load()
    buf = np.full((1, 64), 0xA5, np.uint8)
    p = buf.ctypes.data
    for name in MSG_CALLS + ("c25519_ExpandMessageXmd",):
        extra = (64,) if name == "c25519_ExpandMessageXmd" else ()
        for form, tail in (("_batch", (1,)), ("_dev", (1, None))):
            for args in ((None, p, 8, DST), (p, None, 8, DST), (p, p, 8, None)):
                assert getattr(lib, name + form)(*args, len(DST), *extra, *tail) != 0, (name, form, args)
                assert b"null pointer" in lib.c25519_amd_last_error(), (name, form, args)
    for form, tail in (("_batch", (1,)), ("_dev", (1, None))):
        for args in ((None, p), (p, None)):
            assert getattr(lib, "ed25519_MapToCurve" + form)(*args, *tail) != 0
            assert b"null pointer" in lib.c25519_amd_last_error()
    assert (buf == 0xA5).all()


def test_lengths_out_of_range_are_refused_with_a_message():
    lib = _lib.load()
    buf, long_dst = np.full((1, 64), 0xA5, np.uint8), bytes(256)
    p = buf.ctypes.data
    for name in MSG_CALLS + ("c25519_ExpandMessageXmd",):
        extra = (64,) if name == "c25519_ExpandMessageXmd" else ()
        for form, tail in (("_batch", (1,)), ("_dev", (1, None))):
            for dst_len in (0, 256):
                assert getattr(lib, name + form)(p, p, 8, long_dst, dst_len, *extra, *tail) != 0, (name, form, dst_len)
                assert b"dst_len" in lib.c25519_amd_last_error(), (name, form, dst_len)
    for form, tail in (("_batch", (1,)), ("_dev", (1, None))):
        for n_bytes in (0, 16321):
            assert getattr(lib, "c25519_ExpandMessageXmd" + form)(p, p, 8, DST, len(DST), n_bytes, *tail) != 0
            assert b"len_in_bytes" in lib.c25519_amd_last_error()
    assert (buf == 0xA5).all()
    with pytest.raises(_lib.EngineError):
        api.ed25519_HashToCurve(np.ones((1, 3), np.uint8), b"")
    with pytest.raises(_lib.EngineError):
        api.c25519_ExpandMessageXmd(np.ones((1, 3), np.uint8), DST, 16321)
