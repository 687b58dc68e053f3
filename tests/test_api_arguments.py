"""CPU suite: the argument checks of every public wrapper of curve25519_amd/api.py, both halves, on tiny well-formed arguments (n = 2)
with one thing wrong at a time.  No device is needed: a malformed argument is a ValueError before the library is asked to compute (on a
machine without a GPU a well-formed call raises EngineError and never returns a result, so a ValueError cannot have come from there).

The numpy half: an input one byte too wide, an input with a row missing.  The torch half: CPU tensors, a non-tensor, and -- on tensors
that claim to be CUDA tensors (a subclass whose is_cuda is True; nothing is launched, the check fails first) -- the wrong dtype for an
int32 / int64 column such as ok, idx or verdict; the ValueError then names the argument.  The two tables name every public callable of
api.py that takes an argument: a new wrapper without a row here fails test_the_tables_name_every_public_wrapper."""
import functools
import inspect

import numpy as np
import pytest

from curve25519_amd import api

N = 2
MSG = 5                                   # odd: a message array with a row missing does not reshape to n rows


# ---- the numpy half --------------------------------------------------------------------------------------------------------------
# name -> {argument: spec}, in any order (the call is made with keywords).  spec: an int = uint8[n, width] rows; ("one", width) = ONE
# record of that width; ("ctxs", width) = uint8[3, width] contexts, not counted in rows; "msg" = uint8[n, MSG] rows of any width;
# "messages" = n bytes objects; "idx" = uint32[n]; ("val", v) or anything else = the value itself.  SHORT: the arguments a missing row of which is an
# error where that is not every row-carrying one -- a fixed-length message array is reshaped to the row count of the call's first
# array, so only the message array itself can be a row short there.
def _verify(msg="msg"):
    return dict(sig=64, pk=32, **{("messages" if msg == "messages" else "msg"): msg})


def _indexed(width, msg="msg", first="ctxs"):
    return {first: ("ctxs", width), "idx": "idx", "sig": 64, ("messages" if msg == "messages" else "msg"): msg}


NUMPY = {
    "curve25519_dh_CreateSharedKey": dict(pk=32, sk=32),
    "curve25519_dh_CreateSharedKey_one_peer": dict(pk=("one", 32), sk=32),
    "curve25519_dh_Peer_Init": dict(pk=32),
    "curve25519_dh_CreateSharedKey_indexed": dict(ctxs=("ctxs", 1600), idx="idx", sk=32),
    "curve25519_dh_CalculatePublicKey": dict(sk=32),
    "ed25519_CreateKeyPair": dict(sk=32),
    "ed25519_ClassifyKey": dict(pk=32),
    "ed25519_PublicKey_to_X25519": dict(pk=32),
    "ed25519_PrivateKey_to_X25519": dict(priv=64),
    "ed25519_ScalarMult": dict(scalar=32, point=32),
    "ed25519_ScalarMultBase": dict(scalar=32),
    "ed25519_PointAdd": dict(p=32, q=32),
    "ed25519_PointSub": dict(p=32, q=32),
    "ristretto255_IsValidPoint": dict(point=32),
    "ristretto255_FromHash": dict(hash=64),
    "ristretto255_ScalarMult": dict(scalar=32, point=32),
    "ristretto255_ScalarMultBase": dict(scalar=32),
    "ristretto255_PointAdd": dict(p=32, q=32),
    "ristretto255_PointSub": dict(p=32, q=32),
    "ed25519_ScalarReduce": dict(s=64),
    "ed25519_ScalarAdd": dict(x=32, y=32),
    "ed25519_ScalarSub": dict(x=32, y=32),
    "ed25519_ScalarMul": dict(x=32, y=32),
    "ed25519_ScalarNegate": dict(s=32),
    "ed25519_ScalarComplement": dict(s=32),
    "ed25519_ScalarMulAdd": dict(a=32, b=32, c=32),
    "ed25519_ScalarInvert": dict(s=32),
    "ed25519_ScalarIsCanonical": dict(s=32),
    "c25519_ExpandMessageXmd": dict(msg="msg", dst=b"DST", len_in_bytes=("val", 48)),
    "ed25519_MapToCurve": dict(u=32),
    "ed25519_HashToCurve": dict(msg="msg", dst=b"DST"),
    "ed25519_EncodeToCurve": dict(msg="msg", dst=b"DST"),
    "ristretto255_HashToGroup": dict(msg="msg", dst=b"DST"),
    "ed25519_HashToScalar": dict(msg="msg", dst=b"DST"),
    "ed25519_VRF_Prove": dict(priv=64, alpha="msg"),
    "ed25519_VRF_Verify": dict(pk=32, proof=80, alpha="msg"),
    "ed25519_VRF_ProofToHash": dict(proof=80),
    "ed25519_SignMessage": dict(priv=64, msg="msg"),
    "ed25519_SignMessage_ragged": dict(priv=64, messages="messages"),
    "ed25519_Sign_Init": dict(priv=64),
    "ed25519_SignMessage_indexed": dict(ctxs=("ctxs", 128), idx="idx", msg="msg"),
    "ed25519_SignMessage_indexed_ragged": dict(ctxs=("ctxs", 128), idx="idx", messages="messages"),
    "ed25519_VerifySignature": _verify(),
    "ed25519_VerifySignature_strict": _verify(),
    "ed25519_VerifySignature_zip215": _verify(),
    "ed25519_VerifySignature_ragged": _verify("messages"),
    "ed25519_VerifySignature_strict_ragged": _verify("messages"),
    "ed25519_VerifySignature_zip215_ragged": _verify("messages"),
    "ed25519_VerifyBatch_zip215": _verify(),
    "ed25519_VerifyBatch_zip215_ragged": _verify("messages"),
    "ed25519_Verify_Init": dict(pk=32),
    "ed25519_Verify_Check": dict(ctx=("one", 2080), sig=64, msg="msg"),
    "ed25519_Verify_Check_strict": dict(ctx=("one", 2080), sig=64, msg="msg"),
    "ed25519_Verify_Check_zip215": dict(ctx=("one", 2080), sig=64, msg="msg"),
    "ed25519_Verify_Check_indexed": _indexed(2080),
    "ed25519_Verify_Check_indexed_ragged": _indexed(2080, "messages"),
    "ed25519_Verify_Check_zip215_indexed": _indexed(2080),
    "ed25519_Verify_Check_zip215_indexed_ragged": _indexed(2080, "messages"),
    "ed25519_VerifyBatch_zip215_indexed": _indexed(32, first="keys"),
    "ed25519_VerifyBatch_zip215_indexed_ragged": _indexed(32, "messages", first="keys"),
}
SHORT = {
    "ed25519_SignMessage": ("msg",),
    "ed25519_SignMessage_indexed": ("msg",),
    "ed25519_Verify_Check": ("msg",),
    "ed25519_Verify_Check_strict": ("msg",),
    "ed25519_Verify_Check_zip215": ("msg",),
}


def _np_value(spec, rows=N, extra=0):
    if isinstance(spec, int):
        return np.zeros((rows, spec + extra), np.uint8)
    if isinstance(spec, tuple) and spec[0] == "val":
        return spec[1]
    if isinstance(spec, tuple):
        return np.zeros((1 if spec[0] == "one" else 3, spec[1] + extra), np.uint8)
    if spec == "msg":
        return np.zeros((rows, MSG), np.uint8)
    if spec == "messages":
        return [b"ab", b"c"][:rows]
    if spec == "idx":
        return np.zeros(rows, np.uint32)
    return spec


def _np_args(name):
    return {k: _np_value(s) for k, s in NUMPY[name].items()}


def _fixed_width(spec):
    return isinstance(spec, int) or (isinstance(spec, tuple) and spec[0] != "val")


def _row_carrying(spec):
    return isinstance(spec, int) or spec in ("msg", "messages", "idx")


@pytest.mark.parametrize("name", sorted(NUMPY))
def test_numpy_wrapper_refuses_an_input_a_byte_too_wide(name):
    wide = [k for k, s in NUMPY[name].items() if _fixed_width(s)]
    if not wide:                          # the hashing calls: rows of any width -- what they refuse is an array that is not 2-D
        with pytest.raises(ValueError):
            getattr(api, name)(**{**_np_args(name), "msg": np.zeros(MSG, np.uint8)})
    for k in wide:
        with pytest.raises(ValueError):
            getattr(api, name)(**{**_np_args(name), k: _np_value(NUMPY[name][k], extra=1)})


@pytest.mark.parametrize("name", sorted(NUMPY))
def test_numpy_wrapper_refuses_an_input_with_a_row_missing(name):
    carrying = [k for k, s in NUMPY[name].items() if _row_carrying(s)]
    short = SHORT.get(name, carrying if len(carrying) > 1 else [])
    assert set(short) <= set(carrying)
    for k in short:
        with pytest.raises(ValueError):
            getattr(api, name)(**{**_np_args(name), k: _np_value(NUMPY[name][k], rows=N - 1)})
    for k, s in NUMPY[name].items():      # ONE peer key, ONE context: two are refused
        if isinstance(s, tuple) and s[0] == "one":
            with pytest.raises(ValueError):
                getattr(api, name)(**{**_np_args(name), k: np.zeros((2, s[1]), np.uint8)})


@pytest.mark.parametrize("name", sorted(NUMPY))
def test_numpy_wrapper_never_returns_without_a_device(name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the well-formed call computes")
    with pytest.raises(api.EngineError):
        getattr(api, name)(**_np_args(name))


# ---- the torch half --------------------------------------------------------------------------------------------------------------
# name -> the tensors in the wrapper's argument order, (argument, rows, width, dtype), then the other arguments as (argument, value).
# rows: "n", "n+1" or a number; dtype: "u8", "i32" or "i64".
def T(arg, width, dtype="u8", rows="n"):
    return (arg, rows, width, dtype)


_OK, _IDX, _VERDICT, _RESULT = T("ok", 1, "i32"), T("idx", 1, "i32"), T("verdict", 1, "i32"), T("result", 1, "i32", 1)
_MSG, _FLAT, _OFFSETS = T("msg", MSG), T("flat", 1, rows=7), T("offsets", 1, "i64", "n+1")
_SEED = ("seed", bytes(32))
_SCALARMULT = [T("q", 32), _OK, T("scalar", 32), T("point", 32)]
_ADD = [T("r", 32), _OK, T("p", 32), T("q", 32)]
_BINARY = [T("z", 32), T("x", 32), T("y", 32)]
_UNARY = [T("r", 32), T("s", 32)]
_VERIFY = [_VERDICT, T("sig", 64), T("pk", 32), _MSG]
_CHECK = [_VERDICT, T("ctx", 2080, rows=1), T("sig", 64), _MSG]
_CHECK_INDEXED = [_VERDICT, T("ctxs", 2080, rows=3), _IDX, T("sig", 64)]
_KEYS_INDEXED = [T("keys", 32, rows=3), _IDX, T("sig", 64)]

TORCH = {
    "curve25519_dh_CreateSharedKey_dev": [T("shared", 32), T("pk", 32), T("sk", 32)],
    "curve25519_dh_CreateSharedKey_one_peer_dev": [T("shared", 32), T("pk", 32, rows=1), T("sk", 32)],
    "curve25519_dh_Peer_Init_dev": [T("ctx", 1600), T("pk", 32)],
    "curve25519_dh_CreateSharedKey_indexed_dev": [T("shared", 32), T("ctxs", 1600, rows=3), _IDX, T("sk", 32)],
    "curve25519_dh_CalculatePublicKey_dev": [T("pk", 32), T("sk", 32)],
    "ed25519_CreateKeyPair_dev": [T("pub", 32), T("priv", 64), T("sk", 32)],
    "ed25519_ClassifyKey_dev": [T("flags", 1, "i32"), T("pk", 32)],
    "ed25519_PublicKey_to_X25519_dev": [T("xpk", 32), _OK, T("pk", 32)],
    "ed25519_PrivateKey_to_X25519_dev": [T("xsk", 32), T("priv", 64)],
    "ed25519_ScalarMult_dev": _SCALARMULT,
    "ed25519_ScalarMultBase_dev": [T("q", 32), T("scalar", 32)],
    "ed25519_PointAdd_dev": _ADD,
    "ed25519_PointSub_dev": _ADD,
    "ristretto255_IsValidPoint_dev": [_OK, T("point", 32)],
    "ristretto255_FromHash_dev": [T("p", 32), T("hash", 64)],
    "ristretto255_ScalarMult_dev": _SCALARMULT,
    "ristretto255_ScalarMultBase_dev": [T("q", 32), T("scalar", 32)],
    "ristretto255_PointAdd_dev": _ADD,
    "ristretto255_PointSub_dev": _ADD,
    "ed25519_ScalarReduce_dev": [T("r", 32), T("s", 64)],
    "ed25519_ScalarAdd_dev": _BINARY,
    "ed25519_ScalarSub_dev": _BINARY,
    "ed25519_ScalarMul_dev": _BINARY,
    "ed25519_ScalarNegate_dev": _UNARY,
    "ed25519_ScalarComplement_dev": _UNARY,
    "ed25519_ScalarMulAdd_dev": [T("r", 32), T("a", 32), T("b", 32), T("c", 32)],
    "ed25519_ScalarInvert_dev": [T("recip", 32), _OK, T("s", 32)],
    "ed25519_ScalarIsCanonical_dev": [_OK, T("s", 32)],
    "c25519_ExpandMessageXmd_dev": [T("out", 48), _MSG, ("dst", b"DST")],
    "ed25519_MapToCurve_dev": [T("p", 32), T("u", 32)],
    "ed25519_HashToCurve_dev": [T("p", 32), _MSG, ("dst", b"DST")],
    "ed25519_EncodeToCurve_dev": [T("p", 32), _MSG, ("dst", b"DST")],
    "ristretto255_HashToGroup_dev": [T("p", 32), _MSG, ("dst", b"DST")],
    "ed25519_HashToScalar_dev": [T("s", 32), _MSG, ("dst", b"DST")],
    "ed25519_VRF_Prove_dev": [T("proof", 80), T("priv", 64), T("alpha", MSG)],
    "ed25519_VRF_Verify_dev": [T("beta", 64), _OK, T("pk", 32), T("proof", 80), T("alpha", MSG)],
    "ed25519_VRF_ProofToHash_dev": [T("beta", 64), _OK, T("proof", 80)],
    "ed25519_SignMessage_dev": [T("sig", 64), T("priv", 64), _MSG],
    "ed25519_Sign_Init_dev": [T("ctx", 128), T("priv", 64)],
    "ed25519_SignMessage_indexed_dev": [T("sig", 64), T("ctxs", 128, rows=3), _IDX, _MSG],
    "ed25519_Verify_Check_indexed_dev": _CHECK_INDEXED + [_MSG],
    "ed25519_Verify_Check_zip215_indexed_dev": _CHECK_INDEXED + [_MSG],
    "ed25519_Verify_Check_zip215_indexed_ragged_dev": _CHECK_INDEXED + [_FLAT, _OFFSETS],
    "ed25519_Verify_Check_dev": _CHECK,
    "ed25519_Verify_Check_strict_dev": _CHECK,
    "ed25519_Verify_Check_zip215_dev": _CHECK,
    "ed25519_VerifySignature_dev": _VERIFY,
    "ed25519_VerifySignature_strict_dev": _VERIFY,
    "ed25519_VerifySignature_zip215_dev": _VERIFY,
    "ed25519_VerifyBatch_zip215_dev": [_RESULT, T("sig", 64), T("pk", 32), _MSG, _SEED],
    "ed25519_VerifyBatch_zip215_ragged_dev": [_RESULT, T("sig", 64), T("pk", 32), _FLAT, _OFFSETS, _SEED],
    "verify_batch_point_dev": [T("out", 32, rows=1), T("sig", 64), T("pk", 32), _MSG, _SEED],
    "ed25519_VerifyBatch_zip215_indexed_dev": [_RESULT] + _KEYS_INDEXED + [_MSG, _SEED],
    "ed25519_VerifyBatch_zip215_indexed_ragged_dev": [_RESULT] + _KEYS_INDEXED + [_FLAT, _OFFSETS, _SEED],
    "verify_batch_indexed_point_dev": [T("out", 32, rows=1)] + _KEYS_INDEXED + [_MSG, _SEED],
}


@functools.lru_cache(maxsize=None)
def _claims_cuda():
    import torch

    class ClaimsCuda(torch.Tensor):       # passes the wrappers' `is_cuda` test; its memory is the host's and nothing is launched on it
        is_cuda = property(lambda self: True)

    return ClaimsCuda


def _tensor(spec, cuda, dtype=None):
    import torch
    _, rows, width, dt = spec
    rows = {"n": N, "n+1": N + 1}.get(rows, rows)
    t = torch.zeros((rows, width), dtype={"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}[dtype or dt])
    return torch.Tensor._make_subclass(_claims_cuda(), t) if cuda else t


def _torch_args(name, cuda):
    return {s[0]: (_tensor(s, cuda) if len(s) == 4 else s[1]) for s in TORCH[name]}


@pytest.mark.parametrize("name", sorted(TORCH))
def test_torch_wrapper_refuses_cpu_tensors(name):
    with pytest.raises(ValueError):
        getattr(api, name)(**_torch_args(name, cuda=False))


@pytest.mark.parametrize("name", sorted(TORCH))
def test_torch_wrapper_refuses_a_non_tensor(name):
    for s in TORCH[name]:
        if len(s) == 4:
            with pytest.raises(ValueError):
                getattr(api, name)(**{**_torch_args(name, cuda=False), s[0]: None})
            with pytest.raises(ValueError):
                getattr(api, name)(**{**_torch_args(name, cuda=True), s[0]: [[0] * s[2]] * N})


@pytest.mark.parametrize("name", sorted(TORCH))
def test_torch_wrapper_refuses_a_wrong_dtype(name):
    """uint8 where the column is int32 / int64 (ok, idx, verdict, flags, result, offsets), and int32 for the first uint8 tensor"""
    specs = [s for s in TORCH[name] if len(s) == 4]
    wrong = [(s, "u8") for s in specs if s[3] != "u8"] + [(next(s for s in specs if s[3] == "u8"), "i32")]
    for s, dtype in wrong:
        with pytest.raises(ValueError, match=rf"^{s[0]} must be a contiguous"):
            getattr(api, name)(**{**_torch_args(name, cuda=True), s[0]: _tensor(s, True, dtype)})


# ---- the tables are complete --------------------------------------------------------------------------------------------------------
def test_the_tables_name_every_public_wrapper():
    public = sorted(n for n, f in vars(api).items()
                    if inspect.isfunction(f) and f.__module__ == api.__name__ and not n.startswith("_") and inspect.signature(f).parameters)
    assert public == sorted(list(NUMPY) + list(TORCH))
    assert all(n.endswith("_dev") for n in TORCH) and not any(n.endswith("_dev") for n in NUMPY)
    for name, row in list(NUMPY.items()) + [(n, {s[0]: s for s in r}) for n, r in TORCH.items()]:
        params = inspect.signature(getattr(api, name)).parameters
        required = [p for p, v in params.items() if v.default is inspect.Parameter.empty]
        assert set(required) <= set(row) <= set(params), (name, required, sorted(row))
