"""RFC 9497's OPRF (mode 0x00) and VOPRF (mode 0x01) on ristretto255-SHA512: the host-memory (numpy) and device-memory (torch) forms
of ristretto255_OPRF_Blind, ristretto255_OPRF_Finalize, ristretto255_OPRF_BlindEvaluate, ristretto255_VOPRF_BlindEvaluate and
ristretto255_VOPRF_VerifyProof (include/curve25519_amd.h states their rules), built on api._call / api._dev_call.  Nothing here
computes: without the HIP library and a gfx950 device every call raises EngineError.

    blinded, ok = oprf.ristretto255_OPRF_Blind(inputs, blinds, mode=1)                      # client
    evaluated, proof, ok, req_ok = oprf.ristretto255_VOPRF_BlindEvaluate(skS, r, blinded, offsets)   # server
    req_ok = oprf.ristretto255_VOPRF_VerifyProof(pkS, blinded, evaluated, proof, offsets)  # client
    output, ok = oprf.ristretto255_OPRF_Finalize(inputs, blinds, evaluated)

The blinds and proof_rand are the caller's: uniform, secret, and each used once."""
import numpy as np

from . import _lib
from .api import _B32, _B64, _I32, _I64, _OK, _SIZED, _U8, _call, _dev_call, _np, _ptr
from ._lib import EngineError  # noqa: F401  (re-export)

MODE_OPRF, MODE_VOPRF = 0, 1
MAX_INPUT_SIZE = 65535
MAX_ROWS = 65535                          # of one proof


def _mode(mode):
    if mode not in (MODE_OPRF, MODE_VOPRF):
        raise ValueError(f"mode must be 0 (OPRF) or 1 (VOPRF), got {mode!r}")
    return int(mode)


def _inputs(inp, n):
    """input uint8[n, input_size]: the rows of a call's inputs (input_size may be 0, at most 65535)"""
    inp = np.ascontiguousarray(inp, dtype=np.uint8)
    if inp.ndim != 2 or inp.shape[0] != n:
        raise ValueError(f"input must have shape ({n}, input_size), got {inp.shape}")
    if inp.shape[1] > MAX_INPUT_SIZE:
        raise ValueError(f"input_size must be at most {MAX_INPUT_SIZE}, got {inp.shape[1]}")
    return inp


def _input_dev(inp):
    """the input tensor of a device form, before its width is passed on as input_size: 2-D, at most 65535 bytes a row"""
    import torch
    if not (isinstance(inp, torch.Tensor) and inp.dim() == 2):
        raise ValueError("input must be a 2-D CUDA tensor")
    if inp.shape[1] > MAX_INPUT_SIZE:
        raise ValueError(f"input_size must be at most {MAX_INPUT_SIZE}, got {inp.shape[1]}")
    return inp


def _one(key, name):
    key = _np(key, 32, name)
    if key.shape[0] != 1:
        raise ValueError(f"{name} must be ONE 32-byte string")
    return key


def _offsets(offsets, m, n):
    """uint64[m + 1] from 0 to n in requests of 1 .. 65535 rows (the library checks the same and refuses the call)"""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
    if offsets.shape[0] != m + 1:
        raise ValueError(f"offsets must have {m + 1} entries for {m} requests, got {offsets.shape[0]}")
    sizes = np.diff(offsets.astype(np.int64))
    if int(offsets[0]) != 0 or int(offsets[-1]) != n or (sizes < 1).any() or (sizes > MAX_ROWS).any():
        raise ValueError(f"offsets must rise from 0 to {n} in requests of 1 .. {MAX_ROWS} rows")
    return offsets


# ---- host-memory (numpy) interface ---------------------------------------------------------------
def ristretto255_OPRF_Blind(inp, blind, mode=MODE_OPRF):
    """n x Blind: input uint8[n, input_size], blind uint8[n, 32] (read mod L).  Returns (blinded uint8[n, 32], ok int32[n]):
    blinded = blind * HashToGroup(input) under the mode's context string; ok = 0 where that is the identity (blind = 0 mod L)."""
    blind = _np(blind, 32, "blind")
    inp = _inputs(inp, blind.shape[0])
    return _call("ristretto255_OPRF_Blind_batch", (_ptr(inp) if inp.shape[1] else None, inp.shape[1], (blind, "blind", 32), _mode(mode)), (_B32, _OK))


def ristretto255_OPRF_Finalize(inp, blind, evaluated):
    """n x Finalize: returns (output uint8[n, 64], ok int32[n]): SHA-512(lp(input) || lp((1 / blind) * evaluated) || "Finalize"); ok = 0
    and zeros where evaluated does not decode or is the identity, or blind = 0 mod L."""
    blind = _np(blind, 32, "blind")
    inp = _inputs(inp, blind.shape[0])
    return _call("ristretto255_OPRF_Finalize_batch",
                 (_ptr(inp) if inp.shape[1] else None, inp.shape[1], (blind, "blind", 32), (evaluated, "evaluated", 32)), (_B64, _OK))


def ristretto255_OPRF_BlindEvaluate(skS, blinded):
    """n x BlindEvaluate under ONE key skS (32 bytes): returns (evaluated uint8[n, 32], ok int32[n]); ok = 0 and zeros where the row
    does not decode or it or the result is the identity."""
    skS = _one(skS, "skS")
    return _call("ristretto255_OPRF_BlindEvaluate_batch", (_ptr(skS), (blinded, "blinded", 32)), (_B32, _OK))


def ristretto255_VOPRF_BlindEvaluate(skS, proof_rand, blinded, offsets):
    """m requests over n rows under ONE key: proof_rand uint8[m, 32], blinded uint8[n, 32], offsets uint64[m + 1] (request j owns rows
    offsets[j] .. offsets[j+1] - 1, 1 .. 65535 of them).  Returns (evaluated uint8[n, 32], proof uint8[m, 64], ok int32[n],
    req_ok int32[m]); req_ok = 0 and a zero proof where a row of the request is rejected or proof_rand = 0 or skS = 0 mod L."""
    skS = _one(skS, "skS")
    proof_rand, blinded = _np(proof_rand, 32, "proof_rand"), _np(blinded, 32, "blinded")
    m, n = proof_rand.shape[0], blinded.shape[0]
    offsets = _offsets(offsets, m, n)
    evaluated, proof = np.empty((n, 32), np.uint8), np.empty((m, 64), np.uint8)
    ok, req_ok = np.empty(n, np.int32), np.empty(m, np.int32)
    _lib.check(_lib.load().ristretto255_VOPRF_BlindEvaluate_batch(_ptr(evaluated), _ptr(proof), _ptr(ok), _ptr(req_ok), _ptr(skS), _ptr(proof_rand),
                                                                  _ptr(blinded), _ptr(offsets), m, n), "ristretto255_VOPRF_BlindEvaluate_batch")
    return evaluated, proof, ok, req_ok


def ristretto255_VOPRF_VerifyProof(pkS, blinded, evaluated, proof, offsets):
    """req_ok int32[m]: 1 where proof[j] (uint8[m, 64]) holds for the rows of request j under pkS (32 bytes)."""
    pkS = _one(pkS, "pkS")
    blinded, evaluated, proof = _np(blinded, 32, "blinded"), _np(evaluated, 32, "evaluated"), _np(proof, 64, "proof")
    m, n = proof.shape[0], blinded.shape[0]
    if evaluated.shape[0] != n:
        raise ValueError(f"evaluated must have {n} rows like blinded, got {evaluated.shape[0]}")
    offsets = _offsets(offsets, m, n)
    req_ok = np.empty(m, np.int32)
    _lib.check(_lib.load().ristretto255_VOPRF_VerifyProof_batch(_ptr(req_ok), _ptr(pkS), _ptr(blinded), _ptr(evaluated), _ptr(proof), _ptr(offsets),
                                                                m, n), "ristretto255_VOPRF_VerifyProof_batch")
    return req_ok


def ristretto255_VOPRF_scratch_bytes(m, n):
    """device scratch a proof call leases for m requests over n rows"""
    return int(_lib.load().ristretto255_VOPRF_scratch_bytes(int(m), int(n)))


# ---- device-memory (torch) interface: asynchronous on torch's current stream ----------------------------
def ristretto255_OPRF_Blind_dev(blinded, ok, inp, blind, mode=MODE_OPRF):
    """Device form of ristretto255_OPRF_Blind: input uint8[n, input_size], blind, blinded uint8[n, 32], ok int32[n, 1]."""
    _dev_call("ristretto255_OPRF_Blind_dev", 0, (blinded, "blinded", 32), (ok, "ok", 1, _I32), (_input_dev(inp), "input", _SIZED),
              (blind, "blind", 32), _mode(mode))


def ristretto255_OPRF_Finalize_dev(output, ok, inp, blind, evaluated):
    """Device form of ristretto255_OPRF_Finalize: output uint8[n, 64], ok int32[n, 1], input uint8[n, input_size], blind and evaluated
    uint8[n, 32]."""
    _dev_call("ristretto255_OPRF_Finalize_dev", 0, (output, "output", 64), (ok, "ok", 1, _I32), (_input_dev(inp), "input", _SIZED), (blind, "blind", 32),
              (evaluated, "evaluated", 32))


def ristretto255_OPRF_BlindEvaluate_dev(evaluated, ok, skS, blinded):
    """Device form of ristretto255_OPRF_BlindEvaluate: skS uint8[1, 32] in device memory, blinded, evaluated uint8[n, 32], ok int32[n, 1]."""
    _dev_call("ristretto255_OPRF_BlindEvaluate_dev", 0, (evaluated, "evaluated", 32), (ok, "ok", 1, _I32), (skS, "skS", 32, _U8, 1),
              (blinded, "blinded", 32))


def ristretto255_VOPRF_BlindEvaluate_dev(evaluated, proof, ok, req_ok, skS, proof_rand, blinded, offsets):
    """Device form of ristretto255_VOPRF_BlindEvaluate: evaluated, blinded uint8[n, 32], proof uint8[m, 64], ok int32[n, 1], req_ok
    int32[m, 1], skS uint8[1, 32], proof_rand uint8[m, 32], offsets int64[m + 1, 1] (read as uint64; not trusted: a request that is
    not 1 .. 65535 rows inside [0, n] gets req_ok = 0)."""
    import torch
    if not (isinstance(proof_rand, torch.Tensor) and proof_rand.dim() == 2):
        raise ValueError("proof_rand must be a 2-D CUDA tensor")
    m = proof_rand.shape[0]
    _dev_call("ristretto255_VOPRF_BlindEvaluate_dev", 0, (evaluated, "evaluated", 32), (proof, "proof", 64, _U8, m), (ok, "ok", 1, _I32),
              (req_ok, "req_ok", 1, _I32, m), (skS, "skS", 32, _U8, 1), (proof_rand, "proof_rand", 32, _U8, m), (blinded, "blinded", 32),
              (offsets, "offsets", 1, _I64, m + 1), m)


def ristretto255_VOPRF_VerifyProof_dev(req_ok, pkS, blinded, evaluated, proof, offsets):
    """Device form of ristretto255_VOPRF_VerifyProof: req_ok int32[m, 1], pkS uint8[1, 32], blinded, evaluated uint8[n, 32], proof
    uint8[m, 64], offsets int64[m + 1, 1] (read as uint64; not trusted)."""
    import torch
    if not (isinstance(proof, torch.Tensor) and proof.dim() == 2):
        raise ValueError("proof must be a 2-D CUDA tensor")
    m = proof.shape[0]
    _dev_call("ristretto255_VOPRF_VerifyProof_dev", 2, (req_ok, "req_ok", 1, _I32, m), (pkS, "pkS", 32, _U8, 1), (blinded, "blinded", 32),
              (evaluated, "evaluated", 32), (proof, "proof", 64, _U8, m), (offsets, "offsets", 1, _I64, m + 1), m)
