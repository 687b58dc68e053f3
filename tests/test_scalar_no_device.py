"""The scalar calls at the drop-in boundary without a device: every call fails with an error code and a message (EngineError through
curve25519_amd.api), there is no CPU result behind them, and n == 0 returns 0 all the same.  With a GPU present the first half does
not apply and only the n == 0 and null-pointer rules are checked here (tests/test_gpu_scalar.py holds the rest)."""
import numpy as np
import pytest

from curve25519_amd import _lib, api

CALLS = {   # name: (the widths of the byte inputs, does it write an ok array)
    "ed25519_ScalarReduce": ((64,), False), "ed25519_ScalarAdd": ((32, 32), False), "ed25519_ScalarSub": ((32, 32), False),
    "ed25519_ScalarMul": ((32, 32), False), "ed25519_ScalarNegate": ((32,), False), "ed25519_ScalarComplement": ((32,), False),
    "ed25519_ScalarMulAdd": ((32, 32, 32), False), "ed25519_ScalarInvert": ((32,), True),
}


def has_device():
    return _lib.load().c25519_amd_device_count() > 0


def test_without_a_device_invert_and_mul_raise():
    if has_device():
        assert api.ed25519_ScalarMul(np.ones((2, 32), np.uint8), np.ones((2, 32), np.uint8)).shape == (2, 32)
        return
    s = np.ones((2, 32), np.uint8)
    with pytest.raises(_lib.EngineError):
        api.ed25519_ScalarInvert(s)
    assert _lib.load().c25519_amd_last_error() != b""
    with pytest.raises(_lib.EngineError):
        api.ed25519_ScalarMul(s, s)
    assert _lib.load().c25519_amd_last_error() != b""


def test_without_a_device_no_call_leaves_a_result():
    if has_device():
        return
    for name, (widths, _) in CALLS.items():
        with pytest.raises(_lib.EngineError):
            getattr(api, name)(*[np.ones((3, w), np.uint8) for w in widths])
    with pytest.raises(_lib.EngineError):
        api.ed25519_ScalarIsCanonical(np.ones((3, 32), np.uint8))
    lib = _lib.load()
    out, ok, s = np.full((3, 32), 0xA5, np.uint8), np.full(3, 7, np.int32), np.ones((3, 32), np.uint8)
    assert lib.ed25519_ScalarInvert_batch(out.ctypes.data, ok.ctypes.data, s.ctypes.data, 3) != 0
    assert (out == 0xA5).all() and (ok == 7).all(), "a failed call writes no result"
    assert lib.ed25519_ScalarInvert_dev(out.ctypes.data, ok.ctypes.data, s.ctypes.data, 3, None) != 0


def test_a_call_of_nothing_returns_zero():
    lib = _lib.load()
    buf = np.full((1, 64), 0xA5, np.uint8)
    ok = np.full(1, 7, np.int32)
    p, q = buf.ctypes.data, ok.ctypes.data
    for name, (widths, with_ok) in CALLS.items():
        args = [p] + ([q] if with_ok else []) + [p] * len(widths)
        assert getattr(lib, name + "_batch")(*args, 0) == 0, name
    assert lib.ed25519_ScalarIsCanonical_batch(q, p, 0) == 0
    assert (buf == 0xA5).all() and (ok == 7).all()
    r, k = api.ed25519_ScalarInvert(np.zeros((0, 32), np.uint8))
    assert r.shape == (0, 32) and k.shape == (0,)
    assert api.ed25519_ScalarMul(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8)).shape == (0, 32)


def test_a_null_pointer_is_an_argument_error():
    lib = _lib.load()
    buf = np.full((1, 64), 0xA5, np.uint8)
    ok = np.full(1, 7, np.int32)
    p, q = buf.ctypes.data, ok.ctypes.data
    for name, (widths, with_ok) in CALLS.items():
        args = [p] + ([q] if with_ok else []) + [p] * len(widths)
        for k in range(len(args)):
            for form, tail in (("_batch", (1,)), ("_dev", (1, None))):
                assert getattr(lib, name + form)(*[None if i == k else a for i, a in enumerate(args)], *tail) != 0, (name, form, k)
                assert b"null pointer" in lib.c25519_amd_last_error(), (name, form, k)
    assert (buf == 0xA5).all() and (ok == 7).all()
