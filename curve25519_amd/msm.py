"""Multiscalar multiplication, Q = sum_i [s_i mod L] P_i, on edwards25519 and ristretto255: the host-memory (numpy) and device-memory
(torch) forms of ed25519_MultiScalarMult, ed25519_MultiScalarMult_vartime, ristretto255_MultiScalarMult and
ristretto255_MultiScalarMult_vartime (include/curve25519_amd.h states their rules), built on api._np / api._dev_call.  Nothing here
computes: without the HIP library and a gfx950 device every call raises EngineError.

    q, ok = msm.ristretto255_MultiScalarMult(scalar, point, m)            # n_groups sums of m terms, SECRET scalars
    q, ok = msm.ed25519_MultiScalarMult_vartime(scalar, point, m)         # PUBLIC inputs only
    msm.ristretto255_MultiScalarMult_dev(q, ok, scalar, point)            # torch tensors: m is the ratio of the row counts"""
import numpy as np

from . import _lib
from .api import _I32, _U8, _dev_call, _np, _ptr
from ._lib import EngineError  # noqa: F401  (re-export)

MULTISCALAR_MAX_M = 1 << 26               # rows of one group (c25519_multiscalar_max_m)


def _multiscalar(symbol, scalar, point, m):
    """n_groups sums of m terms: scalar, point uint8[n_groups * m, 32] -> (q uint8[n_groups, 32], ok int32[n_groups])"""
    scalar, point = _np(scalar, 32, "scalar"), _np(point, 32, "point")
    m = int(m)
    if not 1 <= m <= MULTISCALAR_MAX_M:
        raise ValueError(f"m must be 1 .. {MULTISCALAR_MAX_M}, got {m}")
    if point.shape[0] != scalar.shape[0] or scalar.shape[0] % m:
        raise ValueError(f"scalar and point must have the same number of rows, a multiple of m = {m}; got {scalar.shape[0]} and {point.shape[0]}")
    n_groups = scalar.shape[0] // m
    q, ok = np.empty((n_groups, 32), np.uint8), np.empty(n_groups, np.int32)
    _lib.check(getattr(_lib.load(), symbol)(_ptr(q), _ptr(ok), _ptr(scalar), _ptr(point), m, n_groups), symbol)
    return q, ok


def ed25519_MultiScalarMult(scalar, point, m):
    """n_groups x (sum of m terms [s_i mod L] P_i) on edwards25519, SECRET scalars: group g owns rows g m .. g m + m - 1.  Returns
    (q uint8[n_groups, 32], ok int32[n_groups]): ok = 1 and the canonical encoding of the sum where all m points decode (ZIP-215
    decoding), ok = 0 and 32 zero bytes where one does not.  The scalar is all 256 bits, reduced mod L."""
    return _multiscalar("ed25519_MultiScalarMult_batch", scalar, point, m)


def ed25519_MultiScalarMult_vartime(scalar, point, m):
    """ed25519_MultiScalarMult for PUBLIC scalars and points: the same bytes, in time and with memory accesses that depend on the scalars."""
    return _multiscalar("ed25519_MultiScalarMult_vartime_batch", scalar, point, m)


def ristretto255_MultiScalarMult(scalar, point, m):
    """n_groups x (sum of m terms [s_i mod L] P_i) on ristretto255, SECRET scalars.  Returns (q uint8[n_groups, 32], ok int32[n_groups]):
    ok = 1 and ENCODE of the sum where all m points decode (the identity is 32 zero bytes), ok = 0 and zeros where one does not."""
    return _multiscalar("ristretto255_MultiScalarMult_batch", scalar, point, m)


def ristretto255_MultiScalarMult_vartime(scalar, point, m):
    """ristretto255_MultiScalarMult for PUBLIC scalars and points: the same bytes, in time and with memory accesses that depend on the
    scalars."""
    return _multiscalar("ristretto255_MultiScalarMult_vartime_batch", scalar, point, m)


def c25519_MultiScalarMult_scratch_bytes(m, n_groups, vartime=False):
    """device scratch a multiscalar call leases for n_groups sums of m terms (under the current tunables; 0 for sizes it refuses)"""
    return int(_lib.load().c25519_MultiScalarMult_scratch_bytes(int(m), int(n_groups), 1 if vartime else 0))


# ---- device-memory (torch) interface: asynchronous on torch's current stream ----------------------------
def _multiscalar_dev(symbol, q, ok, scalar, point):
    """q uint8[n_groups, 32], ok int32[n_groups, 1], scalar and point uint8[n_groups * m, 32]: m is the ratio of the row counts"""
    import torch
    if not all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in (q, scalar)):
        raise ValueError("q and scalar must be 2-D CUDA tensors")
    n_groups, rows = q.shape[0], scalar.shape[0]
    if n_groups == 0 or rows == 0 or rows % n_groups:
        raise ValueError(f"scalar must have a positive multiple of q's {n_groups} rows, got {rows}")
    _dev_call(symbol, 0, (q, "q", 32), (ok, "ok", 1, _I32), (scalar, "scalar", 32, _U8, rows), (point, "point", 32, _U8, rows), rows // n_groups)


def ed25519_MultiScalarMult_dev(q, ok, scalar, point):
    """Device form of ed25519_MultiScalarMult: q uint8[n_groups, 32], ok int32[n_groups, 1], scalar and point uint8[n_groups * m, 32];
    asynchronous on torch's current stream."""
    _multiscalar_dev("ed25519_MultiScalarMult_dev", q, ok, scalar, point)


def ed25519_MultiScalarMult_vartime_dev(q, ok, scalar, point):
    """Device form of ed25519_MultiScalarMult_vartime (PUBLIC inputs only); asynchronous on torch's current stream."""
    _multiscalar_dev("ed25519_MultiScalarMult_vartime_dev", q, ok, scalar, point)


def ristretto255_MultiScalarMult_dev(q, ok, scalar, point):
    """Device form of ristretto255_MultiScalarMult: q uint8[n_groups, 32], ok int32[n_groups, 1], scalar and point
    uint8[n_groups * m, 32]; asynchronous on torch's current stream."""
    _multiscalar_dev("ristretto255_MultiScalarMult_dev", q, ok, scalar, point)


def ristretto255_MultiScalarMult_vartime_dev(q, ok, scalar, point):
    """Device form of ristretto255_MultiScalarMult_vartime (PUBLIC inputs only); asynchronous on torch's current stream."""
    _multiscalar_dev("ristretto255_MultiScalarMult_vartime_dev", q, ok, scalar, point)
