"""The ECVRF calls at the drop-in boundary without a device: every call fails with an error code and a message (EngineError through
curve25519_amd.api), there is no CPU result behind them and the output buffers stay as they were, and n == 0 returns 0 all the same.
A null pointer is refused with a message before any device is asked for (alpha may be null when alpha_size is 0).  With a GPU
present the first half does not apply and only the argument rules are checked here (tests/test_gpu_vrf.py holds the rest)."""
import numpy as np
import pytest

from curve25519_amd import _lib, api


def has_device():
    return _lib.load().c25519_amd_device_count() > 0


def test_without_a_device_every_call_raises():
    priv, pk, proof, alpha = (np.ones((2, w), np.uint8) for w in (64, 32, 80, 5))
    if has_device():
        assert api.ed25519_VRF_ProofToHash(proof)[0].shape == (2, 64)
        return
    for call in (lambda: api.ed25519_VRF_Prove(priv, alpha), lambda: api.ed25519_VRF_Verify(pk, proof, alpha),
                 lambda: api.ed25519_VRF_ProofToHash(proof), lambda: api.ed25519_VRF_Prove(priv, np.zeros((2, 0), np.uint8))):
        with pytest.raises(_lib.EngineError):
            call()
        assert _lib.load().c25519_amd_last_error() != b""


def test_without_a_device_no_call_leaves_a_result():
    if has_device():
        return
    lib = _lib.load()
    out, ok, src = np.full((3, 80), 0xA5, np.uint8), np.full(3, 0x5A5A5A5A, np.int32), np.ones((3, 80), np.uint8)
    o, k, s = out.ctypes.data, ok.ctypes.data, src.ctypes.data
    assert lib.ed25519_VRF_Prove_batch(o, s, s, 8, 3) != 0 and lib.ed25519_VRF_Prove_dev(o, s, s, 8, 3, None) != 0
    assert lib.ed25519_VRF_Prove_batch(o, s, None, 0, 3) != 0 and lib.ed25519_VRF_Prove_dev(o, s, None, 0, 3, None) != 0
    assert lib.ed25519_VRF_Verify_batch(o, k, s, s, s, 8, 3) != 0 and lib.ed25519_VRF_Verify_dev(o, k, s, s, s, 8, 3, None) != 0
    assert lib.ed25519_VRF_Verify_batch(o, k, s, s, None, 0, 3) != 0
    assert lib.ed25519_VRF_ProofToHash_batch(o, k, s, 3) != 0 and lib.ed25519_VRF_ProofToHash_dev(o, k, s, 3, None) != 0
    assert lib.c25519_amd_last_error() != b""
    assert (out == 0xA5).all() and (ok == 0x5A5A5A5A).all(), "a failed call writes no result"
    assert (src == 1).all()


def test_a_call_of_nothing_returns_zero():
    lib = _lib.load()
    buf = np.full((1, 80), 0xA5, np.uint8)
    p = buf.ctypes.data
    assert lib.ed25519_VRF_Prove_batch(p, p, p, 8, 0) == 0 and lib.ed25519_VRF_Prove_dev(p, p, p, 8, 0, None) == 0
    assert lib.ed25519_VRF_Prove_batch(p, p, None, 0, 0) == 0, "alpha may be NULL when alpha_size is 0"
    assert lib.ed25519_VRF_Verify_batch(p, p, p, p, p, 8, 0) == 0 and lib.ed25519_VRF_Verify_dev(p, p, p, p, p, 8, 0, None) == 0
    assert lib.ed25519_VRF_Verify_batch(p, p, p, p, None, 0, 0) == 0
    assert lib.ed25519_VRF_ProofToHash_batch(p, p, p, 0) == 0 and lib.ed25519_VRF_ProofToHash_dev(p, p, p, 0, None) == 0
    assert (buf == 0xA5).all()
    assert api.ed25519_VRF_Prove(np.zeros((0, 64), np.uint8), np.zeros((0, 7), np.uint8)).shape == (0, 80)
    beta, ok = api.ed25519_VRF_Verify(np.zeros((0, 32), np.uint8), np.zeros((0, 80), np.uint8), np.zeros((0, 7), np.uint8))
    assert beta.shape == (0, 64) and ok.shape == (0,)
    beta, ok = api.ed25519_VRF_ProofToHash(np.zeros((0, 80), np.uint8))
    assert beta.shape == (0, 64) and ok.shape == (0,)


def test_a_null_pointer_is_an_argument_error():
    lib = _lib.load()
    buf = np.full((1, 80), 0xA5, np.uint8)
    p = buf.ctypes.data
    for form, tail in (("_batch", (1,)), ("_dev", (1, None))):
        for args in ((None, p, p, 8), (p, None, p, 8), (p, p, None, 8)):
            assert getattr(lib, "ed25519_VRF_Prove" + form)(*args, *tail) != 0, (form, args)
            assert b"null pointer" in lib.c25519_amd_last_error(), (form, args)
        for args in ((None, p, p, p, p, 8), (p, None, p, p, p, 8), (p, p, None, p, p, 8), (p, p, p, None, p, 8), (p, p, p, p, None, 8)):
            assert getattr(lib, "ed25519_VRF_Verify" + form)(*args, *tail) != 0, (form, args)
            assert b"null pointer" in lib.c25519_amd_last_error(), (form, args)
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert getattr(lib, "ed25519_VRF_ProofToHash" + form)(*args, *tail) != 0, (form, args)
            assert b"null pointer" in lib.c25519_amd_last_error(), (form, args)
    assert (buf == 0xA5).all()


def test_the_wrappers_check_shapes():
    with pytest.raises(ValueError):
        api.ed25519_VRF_Prove(np.zeros((2, 63), np.uint8), np.zeros((2, 4), np.uint8))
    with pytest.raises(ValueError):
        api.ed25519_VRF_Prove(np.zeros((2, 64), np.uint8), np.zeros((3, 4), np.uint8))
    with pytest.raises(ValueError):
        api.ed25519_VRF_Verify(np.zeros((2, 32), np.uint8), np.zeros((3, 80), np.uint8), np.zeros((2, 4), np.uint8))
    with pytest.raises(ValueError):
        api.ed25519_VRF_ProofToHash(np.zeros((2, 64), np.uint8))
