"""Host-side mirror of the reference's operator interface for the scalar-multiplication path.

Function names follow the reference's C API (include/curve25519_dh.h:34-48,
include/ed25519_signature.h:40-93); each takes N-element contiguous arrays and calls the matching
`*_batch` (host memory, numpy) or `*_dev` (device memory, torch CUDA tensors on the current stream)
entry point of libcurve25519_amd.so.  Nothing here computes: no numpy/torch arithmetic, no CPU
fallback -- without the HIP library and a gfx950 device every call raises EngineError.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import EngineError  # noqa: F401  (re-export)


def _np(a, width, name):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 1 and a.size == width:
        a = a.reshape(1, width)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError(f"{name} must have shape (n, {width}), got {a.shape}")
    return a


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _msgs(msg, n):
    msg = np.ascontiguousarray(msg, dtype=np.uint8)
    if n == 0:
        return msg.reshape(0, 0), 0
    msg = msg.reshape(n, -1)
    return msg, msg.shape[1]


# ---- host-memory (numpy) interface ---------------------------------------------------------------
_B32, _B64, _OK = (32, np.uint8), (64, np.uint8), (None, np.int32)     # outputs: uint8[n, 32], uint8[n, 64] and an int32[n] column


def _call(symbol, args, outputs, n=None):
    """One host-memory call, symbol(outputs..., args..., n).  args, in the order of the C prototype: a tuple (array, name, width) is an
    input of n rows of `width` bytes (_np), anything else is passed through as it is.  n is the inputs' row count, which must be the
    same for all of them (and the caller's n where it has one already).  outputs: (width, dtype) each, allocated here as [n, width], or
    as a column [n] for width None.  Returns the output, or the tuple of them.  A wrapper that needs n before the call (to shape its
    messages) runs _np itself and hands the converted array over: _np on it is then a check, not a copy.  A pointer passed through
    (_ptr(msg), _ptr(ctxs)) does not keep its array alive: the wrapper's own local must hold it until this returns."""
    call, keep = [], []
    for a in args:
        if type(a) is tuple:
            arr = _np(a[0], a[2], a[1])
            if n is None:
                n = arr.shape[0]
            elif arr.shape[0] != n:
                raise ValueError(f"{a[1]} must have {n} rows like the other arguments, got {arr.shape[0]}")
            keep.append(arr)
            a = _ptr(arr)
        call.append(a)
    outs = [np.empty(n if w is None else (n, w), dtype) for w, dtype in outputs]
    _lib.check(getattr(_lib.load(), symbol)(*[_ptr(o) for o in outs], *call, n), symbol)
    return outs[0] if len(outs) == 1 else tuple(outs)


def curve25519_dh_CreateSharedKey(pk, sk):
    """n x curve25519_dh_CreateSharedKey.  Returns (shared, clamped_sk); inputs are not modified
    (the C function clamps in place -- the clamped copy is returned instead)."""
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    return _call("curve25519_dh_CreateSharedKey_batch", ((pk, "pk", 32), (sk, "sk", 32)), (_B32,)), sk


def curve25519_dh_CreateSharedKey_one_peer(pk, sk):
    """n x curve25519_dh_CreateSharedKey with ONE peer key `pk` (32 bytes) for every secret.  Returns (shared, clamped_sk);
    the same bytes as curve25519_dh_CreateSharedKey with pk repeated n times (a large call walks a comb built for the peer)."""
    pk = _np(pk, 32, "pk")
    if pk.shape[0] != 1:
        raise ValueError("pk must be ONE 32-byte key")
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    return _call("curve25519_dh_CreateSharedKey_one_peer_batch", (_ptr(pk), (sk, "sk", 32)), (_B32,)), sk


PEER_CTX_SIZE = 1600


def curve25519_dh_Peer_Init(pk):
    """n x curve25519_dh_Peer_Init: peer contexts, uint8[n, 1600] (pk || eligibility || 16 affine rows of 8 * pk's point)."""
    return _call("curve25519_dh_Peer_Init_batch", ((pk, "pk", 32),), ((PEER_CTX_SIZE, np.uint8),))


def curve25519_dh_CreateSharedKey_indexed(ctxs, idx, sk):
    """Many peers in one call: uint8[n_ctx, 1600] contexts (Peer_Init's), uint32[n] indices, n secrets -> (shared, clamped_sk),
    element i against the key of context idx[i] as curve25519_dh_CreateSharedKey would.  An index >= n_ctx raises EngineError."""
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    ctxs, idx = _ctx_index(ctxs, idx, sk.shape[0], PEER_CTX_SIZE, "secret")
    return _call("curve25519_dh_CreateSharedKey_indexed_batch", (_ptr(ctxs), ctxs.shape[0], _ptr(idx), (sk, "sk", 32)), (_B32,)), sk


def x25519_indexed_last_ladder_elements():
    """elements of the calling thread's last CreateSharedKey_indexed call that ran the ladder (-1: no such call); synchronises"""
    return int(_lib.load().c25519_amd_x25519_indexed_last_ladder_elements())


def curve25519_dh_CalculatePublicKey(sk, fast=False):
    """n x curve25519_dh_CalculatePublicKey (or _fast).  Returns (pk, clamped_sk)."""
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    return _call("curve25519_dh_CalculatePublicKey_fast_batch" if fast else "curve25519_dh_CalculatePublicKey_batch", ((sk, "sk", 32),),
                 (_B32,)), sk


def ed25519_CreateKeyPair(sk):
    """n x ed25519_CreateKeyPair(blinding=NULL).  Returns (pub[n,32], priv[n,64])."""
    return _call("ed25519_CreateKeyPair_batch", ((sk, "sk", 32),), (_B32, _B64))


KEY_DECODES, KEY_CANONICAL, KEY_SMALL_ORDER, KEY_TORSION_FREE = 1, 2, 4, 8


def ed25519_ClassifyKey(pk):
    """n x ed25519_ClassifyKey: uint32[n] flags, the OR of KEY_DECODES, KEY_CANONICAL, KEY_SMALL_ORDER and KEY_TORSION_FREE
    (include/curve25519_amd.h states the rule; libsodium's "valid point" is flags == 11)."""
    return _call("ed25519_ClassifyKey_batch", ((pk, "pk", 32),), ((None, np.uint32),))


def ed25519_PublicKey_to_X25519(pk):
    """n x ed25519_PublicKey_to_X25519.  Returns (xpk uint8[n, 32], ok int32[n]): ok = 1 and u = (1 + y) / (1 - y) for a key that
    decodes, is not of small order and is torsion-free; ok = 0 and 32 zero bytes for any other."""
    return _call("ed25519_PublicKey_to_X25519_batch", ((pk, "pk", 32),), (_B32, _OK))


def ed25519_PrivateKey_to_X25519(priv):
    """n x ed25519_PrivateKey_to_X25519: priv uint8[n, 64] (seed || pk) -> uint8[n, 32], the clamped first half of SHA-512(seed)."""
    return _call("ed25519_PrivateKey_to_X25519_batch", ((priv, "priv", 64),), (_B32,))


def ed25519_ScalarMult(scalar, point, clamp=True):
    """n x ed25519_ScalarMult (clamp=False: ed25519_ScalarMult_noclamp).  Returns (q uint8[n, 32], ok int32[n]): ok = 1 and
    q = enc([e]P) where the point bytes decode (the ZIP-215 rule), ok = 0 and 32 zero bytes where they do not; e is the scalar
    clamped on a copy, or its low 255 bits.  The scalar is not modified."""
    return _call("ed25519_ScalarMult_batch" if clamp else "ed25519_ScalarMult_noclamp_batch",
                 ((scalar, "scalar", 32), (point, "point", 32)),
                 (_B32, _OK))


def ed25519_ScalarMultBase(scalar, clamp=True):
    """n x ed25519_ScalarMultBase (clamp=False: ed25519_ScalarMultBase_noclamp): uint8[n, 32], enc([e]B) for every scalar."""
    return _call("ed25519_ScalarMultBase_batch" if clamp else "ed25519_ScalarMultBase_noclamp_batch", ((scalar, "scalar", 32),), (_B32,))


def ed25519_PointAdd(p, q):
    """n x ed25519_PointAdd.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = enc(P + Q) where both decode, else zeros."""
    return _call("ed25519_PointAdd_batch", ((p, "p", 32), (q, "q", 32)), (_B32, _OK))


def ed25519_PointSub(p, q):
    """n x ed25519_PointSub.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = enc(P - Q) where both decode, else zeros."""
    return _call("ed25519_PointSub_batch", ((p, "p", 32), (q, "q", 32)), (_B32, _OK))


def ristretto255_IsValidPoint(point):
    """n x ristretto255_IsValidPoint: int32[n], 1 where the 32 bytes decode by RFC 9496 section 4.3.1."""
    return _call("ristretto255_IsValidPoint_batch", ((point, "point", 32),), (_OK,))


def ristretto255_FromHash(hash):
    """n x ristretto255_FromHash: hash uint8[n, 64] -> uint8[n, 32], ENCODE(MAP(low half) + MAP(high half))."""
    return _call("ristretto255_FromHash_batch", ((hash, "hash", 64),), (_B32,))


def ristretto255_ScalarMult(scalar, point):
    """n x ristretto255_ScalarMult.  Returns (q uint8[n, 32], ok int32[n]): ok = 1 and q = ENCODE([e]P) where the point bytes decode
    (the identity is 32 zero bytes with ok = 1), ok = 0 and 32 zero bytes where they do not; e is the scalar's low 255 bits.  The
    scalar is not modified."""
    return _call("ristretto255_ScalarMult_batch", ((scalar, "scalar", 32), (point, "point", 32)), (_B32, _OK))


def ristretto255_ScalarMultBase(scalar):
    """n x ristretto255_ScalarMultBase: uint8[n, 32], ENCODE([e]B) for every scalar."""
    return _call("ristretto255_ScalarMultBase_batch", ((scalar, "scalar", 32),), (_B32,))


def ristretto255_PointAdd(p, q):
    """n x ristretto255_PointAdd.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = ENCODE(P + Q) where both decode, else zeros."""
    return _call("ristretto255_PointAdd_batch", ((p, "p", 32), (q, "q", 32)), (_B32, _OK))


def ristretto255_PointSub(p, q):
    """n x ristretto255_PointSub.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = ENCODE(P - Q) where both decode, else zeros."""
    return _call("ristretto255_PointSub_batch", ((p, "p", 32), (q, "q", 32)), (_B32, _OK))


def ed25519_ScalarReduce(s):
    """n x ed25519_ScalarReduce: s uint8[n, 64] -> uint8[n, 32], the 512-bit value mod L."""
    return _call("ed25519_ScalarReduce_batch", ((s, "s", 64),), (_B32,))


def ed25519_ScalarAdd(x, y):
    """n x ed25519_ScalarAdd: uint8[n, 32], x + y mod L (canonical; the inputs may be any 32-byte values)."""
    return _call("ed25519_ScalarAdd_batch", ((x, "x", 32), (y, "y", 32)), (_B32,))


def ed25519_ScalarSub(x, y):
    """n x ed25519_ScalarSub: uint8[n, 32], x - y mod L."""
    return _call("ed25519_ScalarSub_batch", ((x, "x", 32), (y, "y", 32)), (_B32,))


def ed25519_ScalarMul(x, y):
    """n x ed25519_ScalarMul: uint8[n, 32], x y mod L."""
    return _call("ed25519_ScalarMul_batch", ((x, "x", 32), (y, "y", 32)), (_B32,))


def ed25519_ScalarNegate(s):
    """n x ed25519_ScalarNegate: uint8[n, 32], -s mod L."""
    return _call("ed25519_ScalarNegate_batch", ((s, "s", 32),), (_B32,))


def ed25519_ScalarComplement(s):
    """n x ed25519_ScalarComplement: uint8[n, 32], 1 - s mod L."""
    return _call("ed25519_ScalarComplement_batch", ((s, "s", 32),), (_B32,))


def ed25519_ScalarMulAdd(a, b, c):
    """n x ed25519_ScalarMulAdd: uint8[n, 32], a b + c mod L."""
    return _call("ed25519_ScalarMulAdd_batch", ((a, "a", 32), (b, "b", 32), (c, "c", 32)), (_B32,))


def ed25519_ScalarInvert(s):
    """n x ed25519_ScalarInvert.  Returns (recip uint8[n, 32], ok int32[n]): ok = 1 and recip = 1 / s mod L where s mod L != 0, ok = 0
    and 32 zero bytes where it is zero (s = L included: zero is judged after reduction)."""
    return _call("ed25519_ScalarInvert_batch", ((s, "s", 32),), (_B32, _OK))


def ed25519_ScalarIsCanonical(s):
    """n x ed25519_ScalarIsCanonical: int32[n], 1 where the 32 bytes are below L."""
    return _call("ed25519_ScalarIsCanonical_batch", ((s, "s", 32),), (_OK,))


def _h2c_args(msg, dst):
    """(msg uint8[n, msg_size], dst as a bytes buffer): the rows of a hashing call and its domain separation tag"""
    msg = np.ascontiguousarray(msg, dtype=np.uint8)
    if msg.ndim != 2:
        raise ValueError(f"msg must have shape (n, msg_size), got {msg.shape}")
    return msg, bytes(dst)


def _h2c_call(name, msg, dst):
    msg, dst = _h2c_args(msg, dst)
    n, msg_size = msg.shape
    return _call(name, (_ptr(msg) if msg_size else None, msg_size, dst, len(dst)), (_B32,), n)


def c25519_ExpandMessageXmd(msg, dst, len_in_bytes):
    """n x expand_message_xmd over SHA-512 (RFC 9380 section 5.3.1): msg uint8[n, msg_size], dst 1 .. 255 bytes ->
    uint8[n, len_in_bytes], 1 <= len_in_bytes <= 16320."""
    msg, dst = _h2c_args(msg, dst)
    n, msg_size = msg.shape
    return _call("c25519_ExpandMessageXmd_batch", (_ptr(msg) if msg_size else None, msg_size, dst, len(dst), int(len_in_bytes)),
                 ((max(int(len_in_bytes), 0), np.uint8),), n)


def ed25519_MapToCurve(u):
    """n x map_to_curve_elligator2_edwards25519 (RFC 9380 section 6.8.2): u uint8[n, 32] (little-endian, bit 255 masked, mod p) ->
    the Ed25519 encodings uint8[n, 32]; no cofactor cleared, u = 0 gives the identity."""
    return _call("ed25519_MapToCurve_batch", ((u, "u", 32),), (_B32,))


def ed25519_HashToCurve(msg, dst):
    """n x edwards25519_XMD:SHA-512_ELL2_RO_ under the DST dst: msg uint8[n, msg_size] -> the Ed25519 encodings uint8[n, 32]."""
    return _h2c_call("ed25519_HashToCurve_batch", msg, dst)


def ed25519_EncodeToCurve(msg, dst):
    """n x edwards25519_XMD:SHA-512_ELL2_NU_ under the DST dst: msg uint8[n, msg_size] -> the Ed25519 encodings uint8[n, 32]."""
    return _h2c_call("ed25519_EncodeToCurve_batch", msg, dst)


def ristretto255_HashToGroup(msg, dst):
    """n x hash_to_ristretto255 (RFC 9380 appendix B; RFC 9497's HashToGroup with dst = "HashToGroup-" || contextString):
    msg uint8[n, msg_size] -> uint8[n, 32]."""
    return _h2c_call("ristretto255_HashToGroup_batch", msg, dst)


def ed25519_HashToScalar(msg, dst):
    """n x RFC 9497's HashToScalar for ristretto255 (dst = "HashToScalar-" || contextString): msg uint8[n, msg_size] -> the
    canonical scalars uint8[n, 32], 64 expander bytes little-endian mod L."""
    return _h2c_call("ed25519_HashToScalar_batch", msg, dst)


def _vrf_alpha(alpha, n):
    """alpha uint8[n, alpha_size]: the rows of a VRF call's inputs (alpha_size may be 0)"""
    alpha = np.ascontiguousarray(alpha, dtype=np.uint8)
    if alpha.ndim != 2 or alpha.shape[0] != n:
        raise ValueError(f"alpha must have shape ({n}, alpha_size), got {alpha.shape}")
    return alpha


def ed25519_VRF_Prove(priv, alpha):
    """n x ECVRF-EDWARDS25519-SHA512-ELL2 prove (RFC 9381 section 5.1): priv uint8[n, 64] (seed || public key, the public half read
    as given), alpha uint8[n, alpha_size] -> the proofs uint8[n, 80], Gamma || c || s."""
    priv = _np(priv, 64, "priv")
    alpha = _vrf_alpha(alpha, priv.shape[0])
    return _call("ed25519_VRF_Prove_batch", ((priv, "priv", 64), _ptr(alpha) if alpha.shape[1] else None, alpha.shape[1]),
                 ((80, np.uint8),))


def ed25519_VRF_Verify(pk, proof, alpha):
    """n x ECVRF verify with validate_key = TRUE (RFC 9381 section 5.3): pk uint8[n, 32], proof uint8[n, 80], alpha
    uint8[n, alpha_size].  Returns (beta uint8[n, 64], ok int32[n]): ok = 1 and the VRF output where the proof is valid, ok = 0 and
    64 zero bytes where it is not."""
    pk = _np(pk, 32, "pk")
    alpha = _vrf_alpha(alpha, pk.shape[0])
    return _call("ed25519_VRF_Verify_batch",
                 ((pk, "pk", 32), (proof, "proof", 80), _ptr(alpha) if alpha.shape[1] else None, alpha.shape[1]),
                 (_B64, _OK))


def ed25519_VRF_ProofToHash(proof):
    """n x ECVRF proof_to_hash (RFC 9381 section 5.2): proof uint8[n, 80].  Returns (beta uint8[n, 64], ok int32[n]): ok = 0 and 64
    zero bytes where the proof does not decode.  The proof is NOT verified."""
    return _call("ed25519_VRF_ProofToHash_batch", ((proof, "proof", 80),), (_B64, _OK))


def ed25519_SignMessage(priv, msg):
    """n x ed25519_SignMessage(blinding=NULL) over fixed-length messages msg[n, msg_size]."""
    priv = _np(priv, 64, "priv")
    msg, msg_size = _msgs(msg, priv.shape[0])
    return _call("ed25519_SignMessage_batch", ((priv, "priv", 64), _ptr(msg), msg_size), (_B64,))


def _ragged(messages):
    """list of bytes-like -> (concatenated uint8 array, uint64 offsets[n+1])"""
    lens = np.fromiter((len(m) for m in messages), dtype=np.uint64, count=len(messages))
    offsets = np.zeros(len(messages) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    flat = np.frombuffer(b"".join(bytes(m) for m in messages), np.uint8) if len(messages) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat), offsets


def ed25519_SignMessage_ragged(priv, messages):
    """n x ed25519_SignMessage with per-element message lengths (`messages`: sequence of bytes-like)."""
    priv = _np(priv, 64, "priv")
    if len(messages) != priv.shape[0]:
        raise ValueError("one message per private key")
    flat, offsets = _ragged(messages)
    return _call("ed25519_SignMessage_ragged_batch", ((priv, "priv", 64), _ptr(flat), _ptr(offsets)), (_B64,))


SIGN_CTX_SIZE = 128


def ed25519_Sign_Init(priv):
    """n x ed25519_Sign_Init: signer contexts, uint8[n, 128] (a || prefix || pk || 0).  As secret as the private keys."""
    return _call("ed25519_Sign_Init_batch", ((priv, "priv", 64),), ((SIGN_CTX_SIZE, np.uint8),))


def ed25519_SignMessage_indexed(ctxs, idx, msg):
    """Many keys in one call: uint8[n_ctx, 128] contexts (Sign_Init's), uint32[n] indices, fixed-length messages msg[n, msg_size] ->
    uint8[n, 64], signature i as ed25519_SignMessage under the key of context idx[i].  An index >= n_ctx raises EngineError."""
    n = np.size(idx)
    ctxs, idx = _ctx_index(ctxs, idx, n, SIGN_CTX_SIZE, "message")
    msg, msg_size = _msgs(msg, n)
    return _call("ed25519_SignMessage_indexed_batch", (_ptr(ctxs), ctxs.shape[0], _ptr(idx), _ptr(msg), msg_size), (_B64,), n)


def ed25519_SignMessage_indexed_ragged(ctxs, idx, messages):
    """ed25519_SignMessage_indexed with per-element message lengths (`messages`: sequence of bytes-like)."""
    n = len(messages)
    ctxs, idx = _ctx_index(ctxs, idx, n, SIGN_CTX_SIZE, "message")
    flat, offsets = _ragged(messages)
    return _call("ed25519_SignMessage_indexed_ragged_batch", (_ptr(ctxs), ctxs.shape[0], _ptr(idx), _ptr(flat), _ptr(offsets)), (_B64,), n)


# the verification rule sets (include/curve25519_amd.h): what goes between "ed25519_VerifySignature_" and the form's suffix
_RULES = {"plain": "", "strict": "strict_", "zip215": "zip215_"}


def _verify_ragged(sig, pk, messages, rules):
    sig = _np(sig, 64, "sig")
    if len(messages) != sig.shape[0]:
        raise ValueError("one message and one key per signature")
    flat, offsets = _ragged(messages)
    return _call(f"ed25519_VerifySignature_{_RULES[rules]}ragged_batch", ((sig, "sig", 64), (pk, "pk", 32), _ptr(flat), _ptr(offsets)),
                 (_OK,))


def ed25519_VerifySignature_ragged(sig, pk, messages, strict=False):
    return _verify_ragged(sig, pk, messages, "strict" if strict else "plain")


def ed25519_VerifySignature_strict_ragged(sig, pk, messages):
    """ed25519_VerifySignature_strict with per-element message lengths (`messages`: sequence of bytes-like)."""
    return _verify_ragged(sig, pk, messages, "strict")


def _verify(sig, pk, msg, rules):
    sig = _np(sig, 64, "sig")
    msg, msg_size = _msgs(msg, sig.shape[0])
    return _call(f"ed25519_VerifySignature_{_RULES[rules]}batch", ((sig, "sig", 64), (pk, "pk", 32), _ptr(msg), msg_size), (_OK,))


def ed25519_VerifySignature_strict(sig, pk, msg):
    """n x strict verification (include/curve25519_amd.h: rules 1-6 -- S < L, a canonical key on the curve and not of small order,
    R not of small order, and the reference's verdict).  Returns int32[n] of 1 (valid) / 0 (invalid or rejected)."""
    return _verify(sig, pk, msg, "strict")


def ed25519_VerifySignature(sig, pk, msg, strict=False):
    """n x ed25519_VerifySignature.  Returns int32[n] of 1 (valid) / 0 (invalid)."""
    return _verify(sig, pk, msg, "strict" if strict else "plain")


def ed25519_VerifySignature_zip215(sig, pk, msg):
    """n x ZIP-215 verification (include/curve25519_amd.h: S < L, key and R in any encoding that decodes, the cofactored equation
    [8]([S]B - [k]A - R) = O).  Returns int32[n] of 1 (valid) / 0 (invalid)."""
    return _verify(sig, pk, msg, "zip215")


def ed25519_VerifySignature_zip215_ragged(sig, pk, messages):
    """ed25519_VerifySignature_zip215 with per-element message lengths (`messages`: sequence of bytes-like)."""
    return _verify_ragged(sig, pk, messages, "zip215")


def _seed(seed):
    """None, or 32 bytes as a ctypes buffer (it must outlive the call)"""
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    return C.create_string_buffer(seed, 32)


def ed25519_VerifyBatch_zip215(sig, pk, msg, seed=None, verdicts=False):
    """ZIP-215 batch verification, one random linear combination per call (include/curve25519_amd.h): 1 if every signature is valid,
    0 otherwise (wrongly 1 with probability at most 2^-128 over the seed).  seed: 32 fresh, unpredictable bytes, or None for
    getrandom(2).  verdicts=True returns (all_valid, int32[n]): all ones, or ed25519_VerifySignature_zip215's verdicts when the batch
    fails."""
    sig = _np(sig, 64, "sig")
    pk = _np(pk, 32, "pk")
    n = sig.shape[0]
    if pk.shape[0] != n:
        raise ValueError("sig and pk must have the same number of rows")
    msg, msg_size = _msgs(msg, n)
    ok = C.c_int(-1)
    verdict = np.empty(n, np.int32) if verdicts else None
    sd = _seed(seed)
    _lib.check(_lib.load().ed25519_VerifyBatch_zip215_batch(C.byref(ok), _ptr(verdict) if verdicts else None, _ptr(sig), _ptr(pk),
                                                            _ptr(msg), msg_size, n, sd), "ed25519_VerifyBatch_zip215_batch")
    return (ok.value, verdict) if verdicts else ok.value


def ed25519_VerifyBatch_zip215_ragged(sig, pk, messages, seed=None, verdicts=False):
    """ed25519_VerifyBatch_zip215 with per-element message lengths (`messages`: sequence of bytes-like)."""
    sig = _np(sig, 64, "sig")
    pk = _np(pk, 32, "pk")
    n = sig.shape[0]
    if len(messages) != n or pk.shape[0] != n:
        raise ValueError("one message and one key per signature")
    flat, offsets = _ragged(messages)
    ok = C.c_int(-1)
    verdict = np.empty(n, np.int32) if verdicts else None
    sd = _seed(seed)
    _lib.check(_lib.load().ed25519_VerifyBatch_zip215_ragged_batch(C.byref(ok), _ptr(verdict) if verdicts else None, _ptr(sig), _ptr(pk),
                                                                   _ptr(flat), _ptr(offsets), n, sd),
               "ed25519_VerifyBatch_zip215_ragged_batch")
    return (ok.value, verdict) if verdicts else ok.value


def verify_batch_last_equation():
    """1: the calling thread's last ed25519_VerifyBatch_zip215 call (indexed or not) ran the equation, 0: the per-element path, -1: no
    such call"""
    return int(_lib.load().c25519_amd_verify_batch_last_equation())


def ed25519_Verify_Init(pk):
    """n x ed25519_Verify_Init: per-key contexts, uint8[n, 2080] (pk || 16 rows x 4 canonical elements)."""
    return _call("ed25519_Verify_Init_batch", ((pk, "pk", 32),), ((2080, np.uint8),))


def ed25519_Verify_Check_strict(ctx, sig, msg):
    """ed25519_Verify_Check under the strict rules (rules 2-4 on the context's key bytes 0..31)."""
    return ed25519_Verify_Check(ctx, sig, msg, strict=True)


def ed25519_Verify_Check_zip215(ctx, sig, msg):
    """The ZIP-215 verdict against one Verify_Init context: for a context that is Verify_Init's, ed25519_VerifySignature_zip215's
    verdict under the context's key bytes 0..31 (include/curve25519_amd.h)."""
    return ed25519_Verify_Check(ctx, sig, msg, rules="zip215")


def ed25519_Verify_Check(ctx, sig, msg, strict=False, rules=None):
    """One key (a 2080-byte context), n (signature, message) pairs -> int32[n] verdicts."""
    ctx = np.ascontiguousarray(ctx, dtype=np.uint8).reshape(-1)
    if ctx.size != 2080:
        raise ValueError("ctx must be one 2080-byte context")
    sig = _np(sig, 64, "sig")
    msg, msg_size = _msgs(msg, sig.shape[0])
    return _call(f"ed25519_Verify_Check_{_RULES[rules or ('strict' if strict else 'plain')]}batch",
                 (_ptr(ctx), (sig, "sig", 64), _ptr(msg), msg_size), (_OK,))


def _ctx_index(ctxs, idx, n, width=2080, what="signature"):
    ctxs = _np(ctxs, width, "ctxs") if np.size(ctxs) else np.zeros((0, width), np.uint8)
    idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
    if idx.size != n:
        raise ValueError(f"one context index per {what}")
    return ctxs, idx


def ed25519_Verify_Check_indexed(ctxs, idx, sig, msg, zip215=False):
    """Many keys in one call: uint8[n_ctx, 2080] contexts (Verify_Init's), uint32[n] indices, n (signature, message) pairs ->
    int32[n], element i checked against context idx[i] as ed25519_Verify_Check would.  An index >= n_ctx raises EngineError."""
    sig = _np(sig, 64, "sig")
    ctxs, idx = _ctx_index(ctxs, idx, sig.shape[0])
    msg, msg_size = _msgs(msg, sig.shape[0])
    return _call("ed25519_Verify_Check_zip215_indexed_batch" if zip215 else "ed25519_Verify_Check_indexed_batch",
                 (_ptr(ctxs), ctxs.shape[0], _ptr(idx), (sig, "sig", 64), _ptr(msg), msg_size), (_OK,))


def ed25519_Verify_Check_indexed_ragged(ctxs, idx, sig, messages, zip215=False):
    """ed25519_Verify_Check_indexed with per-element message lengths (`messages`: sequence of bytes-like)."""
    sig = _np(sig, 64, "sig")
    ctxs, idx = _ctx_index(ctxs, idx, sig.shape[0])
    if len(messages) != sig.shape[0]:
        raise ValueError("one message per signature")
    flat, offsets = _ragged(messages)
    return _call("ed25519_Verify_Check_zip215_indexed_ragged_batch" if zip215 else "ed25519_Verify_Check_indexed_ragged_batch",
                 (_ptr(ctxs), ctxs.shape[0], _ptr(idx), (sig, "sig", 64), _ptr(flat), _ptr(offsets)), (_OK,))


def ed25519_Verify_Check_zip215_indexed(ctxs, idx, sig, msg):
    """ed25519_Verify_Check_indexed under the ZIP-215 rule: element i gets ed25519_VerifySignature_zip215's verdict under the key bytes
    of context idx[i], for contexts that are Verify_Init's (include/curve25519_amd.h).  An index >= n_ctx raises EngineError."""
    return ed25519_Verify_Check_indexed(ctxs, idx, sig, msg, zip215=True)


def ed25519_Verify_Check_zip215_indexed_ragged(ctxs, idx, sig, messages):
    """ed25519_Verify_Check_zip215_indexed with per-element message lengths (`messages`: sequence of bytes-like)."""
    return ed25519_Verify_Check_indexed_ragged(ctxs, idx, sig, messages, zip215=True)


def ed25519_VerifyBatch_zip215_indexed(keys, idx, sig, msg, seed=None, verdicts=False):
    """ed25519_VerifyBatch_zip215 with coalesced keys: uint8[n_key, 32] raw keys, uint32[n] indices, element i verified under
    keys[idx[i]]; the terms of one key are merged into one point of the equation (include/curve25519_amd.h).  The result, and the
    verdicts of verdicts=True, are ed25519_VerifyBatch_zip215's on keys[idx].  An index >= n_key raises EngineError."""
    sig = _np(sig, 64, "sig")
    n = sig.shape[0]
    keys, idx = _ctx_index(keys, idx, n, 32)
    msg, msg_size = _msgs(msg, n)
    ok = C.c_int(-1)
    verdict = np.empty(n, np.int32) if verdicts else None
    sd = _seed(seed)
    _lib.check(_lib.load().ed25519_VerifyBatch_zip215_indexed_batch(C.byref(ok), _ptr(verdict) if verdicts else None, _ptr(keys),
                                                                    keys.shape[0], _ptr(idx), _ptr(sig), _ptr(msg), msg_size, n, sd),
               "ed25519_VerifyBatch_zip215_indexed_batch")
    return (ok.value, verdict) if verdicts else ok.value


def ed25519_VerifyBatch_zip215_indexed_ragged(keys, idx, sig, messages, seed=None, verdicts=False):
    """ed25519_VerifyBatch_zip215_indexed with per-element message lengths (`messages`: sequence of bytes-like)."""
    sig = _np(sig, 64, "sig")
    n = sig.shape[0]
    keys, idx = _ctx_index(keys, idx, n, 32)
    if len(messages) != n:
        raise ValueError("one message per signature")
    flat, offsets = _ragged(messages)
    ok = C.c_int(-1)
    verdict = np.empty(n, np.int32) if verdicts else None
    sd = _seed(seed)
    _lib.check(_lib.load().ed25519_VerifyBatch_zip215_indexed_ragged_batch(C.byref(ok), _ptr(verdict) if verdicts else None, _ptr(keys),
                                                                           keys.shape[0], _ptr(idx), _ptr(sig), _ptr(flat),
                                                                           _ptr(offsets), n, sd),
               "ed25519_VerifyBatch_zip215_indexed_ragged_batch")
    return (ok.value, verdict) if verdicts else ok.value


def last_shape():
    """(form, lanes per workgroup) of the calling thread's last base call -- X25519, public key, key pair, signature, verification --
    or None when there is none (include/curve25519_amd.h: c25519_amd_last_shape).  form: 1 one element per workgroup, 2 four lanes
    per element, 3 one lane per element, 4 one lane per element with the shared inversion as its own launch."""
    v = int(_lib.load().c25519_amd_last_shape())
    return None if v < 0 else (v & 0xFF, v >> 8)


def base_folding8_table():
    """(256, 3, 32) uint8: the device-generated 8-fold base table in the reference's PA_POINT row order."""
    out = np.empty((256, 3, 32), np.uint8)
    _lib.check(_lib.load().c25519_amd_base_table(_ptr(out)), "c25519_amd_base_table")
    return out


def device_count() -> int:
    return int(_lib.load().c25519_amd_device_count())


# ---- device-memory (torch CUDA tensors) interface --------------------------------------------------
# torch is only plumbing here: it owns the HBM buffers and the stream.  Every tensor is checked (CUDA, dtype,
# contiguous, shape, same row count, same device) before its data_ptr() is handed to the C ABI, and the call runs
# with that device current -- a short or strided tensor is a ValueError here, not an out-of-bounds access there.

_U8, _I32, _I64 = "uint8", "int32", "int64"
_SIZED, _COUNTED = "sized", "counted"     # a width / a row count that is not fixed and is passed to the call behind the pointer
_SPEC_DEFAULTS = (_U8, "n")


def _dev_call(symbol, anchor, *args, after=()):
    """One device-memory call on torch's current stream, symbol(args..., n, after..., stream).  args, in the order of the C prototype:
    a tuple (tensor, name, width[, dtype[, rows]]) is a tensor, anything else is passed through as it is.  width: the row's elements,
    None for any, or _SIZED: any, passed behind the pointer (msg, msg_size), a null pointer when it is 0.  rows: "n" (the default),
    "n+1", a number, None for any, or _COUNTED: any, passed behind the pointer (ctxs, n_ctx).  args[anchor] is the tensor whose row
    count is n and whose device is the call's; it is looked at before its shape is read."""
    import torch
    t = args[anchor][0]
    if not (isinstance(t, torch.Tensor) and t.dim() == 2):
        raise ValueError(f"{args[anchor][1]} must be a 2-D CUDA tensor")
    n, device = t.shape[0], t.device
    call = []
    for spec in args:
        if type(spec) is not tuple:
            call.append(spec)
            continue
        t, name, width, dtype, rows = spec + _SPEC_DEFAULTS[len(spec) - 3:]
        dtype = getattr(torch, dtype)
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor")
        if t.dim() != 2 or (type(width) is int and t.shape[1] != width):
            raise ValueError(f"{name} must have shape (n, {width}), got {tuple(t.shape)}")
        want = n if rows == "n" else n + 1 if rows == "n+1" else rows
        if type(want) is int and t.shape[0] != want:
            raise ValueError(f"{name} must have {want} rows, got {t.shape[0]}")
        if t.device != device:
            raise ValueError(f"{name} is on {t.device}, the other arguments on {device}")
        if width is _SIZED:
            call += (C.c_void_p(t.data_ptr()) if t.shape[1] else None, t.shape[1])
        else:
            call.append(C.c_void_p(t.data_ptr()))
        if rows is _COUNTED:
            call.append(t.shape[0])
    with _on(args[anchor][0]) as st:
        _lib.check(getattr(_lib.load(), symbol)(*call, n, *after, st), symbol)


class _on:
    """`with _on(t):` = torch.cuda.device(t.device) + the current stream of that device as a void*."""

    def __init__(self, t):
        import torch
        self.ctx = torch.cuda.device(t.device)

    def __enter__(self):
        import torch
        self.ctx.__enter__()
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)


def curve25519_dh_CreateSharedKey_dev(shared, pk, sk):
    """In-place device form: writes `shared`, clamps `sk`; asynchronous on torch's current stream."""
    _dev_call("curve25519_dh_CreateSharedKey_dev", 1, (shared, "shared", 32), (pk, "pk", 32), (sk, "sk", 32))


def curve25519_dh_CreateSharedKey_one_peer_dev(shared, pk, sk):
    """In-place device form with ONE peer key (`pk`: a (1, 32) or (32,) uint8 CUDA tensor): writes `shared`, clamps `sk`;
    asynchronous on torch's current stream (the comb-or-ladder decision is taken on the device)."""
    pk = pk.reshape(1, -1) if getattr(pk, "dim", lambda: 2)() == 1 else pk
    _dev_call("curve25519_dh_CreateSharedKey_one_peer_dev", 2, (shared, "shared", 32), (pk, "pk", 32, _U8, 1), (sk, "sk", 32))


def curve25519_dh_Peer_Init_dev(ctx, pk):
    """Device form of curve25519_dh_Peer_Init: pk uint8[n, 32], ctx uint8[n, 1600]; asynchronous on torch's current stream."""
    _dev_call("curve25519_dh_Peer_Init_dev", 1, (ctx, "ctx", PEER_CTX_SIZE), (pk, "pk", 32))


def curve25519_dh_CreateSharedKey_indexed_dev(shared, ctxs, idx, sk):
    """Device form of curve25519_dh_CreateSharedKey_indexed: ctxs uint8[n_ctx, 1600], idx int32[n, 1] (read as uint32), writes
    `shared`, clamps `sk`.  An index >= n_ctx gives 32 zero bytes (nothing is checked on the host); does not synchronise."""
    _dev_call("curve25519_dh_CreateSharedKey_indexed_dev", 3, (shared, "shared", 32), (ctxs, "ctxs", PEER_CTX_SIZE, _U8, _COUNTED),
              (idx, "idx", 1, _I32), (sk, "sk", 32))


def curve25519_dh_CalculatePublicKey_dev(pk, sk, fast=False):
    _dev_call("curve25519_dh_CalculatePublicKey_fast_dev" if fast else "curve25519_dh_CalculatePublicKey_dev", 1, (pk, "pk", 32),
              (sk, "sk", 32))


def ed25519_CreateKeyPair_dev(pub, priv, sk):
    _dev_call("ed25519_CreateKeyPair_dev", 2, (pub, "pub", 32), (priv, "priv", 64), (sk, "sk", 32))


def ed25519_ClassifyKey_dev(flags, pk):
    """Device form of ed25519_ClassifyKey: pk uint8[n, 32], flags int32[n, 1] (read as uint32); asynchronous on torch's current stream."""
    _dev_call("ed25519_ClassifyKey_dev", 1, (flags, "flags", 1, _I32), (pk, "pk", 32))


def ed25519_PublicKey_to_X25519_dev(xpk, ok, pk):
    """Device form of ed25519_PublicKey_to_X25519: pk uint8[n, 32], xpk uint8[n, 32], ok int32[n, 1]; asynchronous on torch's
    current stream."""
    _dev_call("ed25519_PublicKey_to_X25519_dev", 2, (xpk, "xpk", 32), (ok, "ok", 1, _I32), (pk, "pk", 32))


def ed25519_PrivateKey_to_X25519_dev(xsk, priv):
    """Device form of ed25519_PrivateKey_to_X25519: priv uint8[n, 64], xsk uint8[n, 32]; asynchronous on torch's current stream."""
    _dev_call("ed25519_PrivateKey_to_X25519_dev", 1, (xsk, "xsk", 32), (priv, "priv", 64))


def ed25519_ScalarMult_dev(q, ok, scalar, point, clamp=True):
    """Device form of ed25519_ScalarMult (clamp=False: _noclamp): scalar, point, q uint8[n, 32], ok int32[n, 1]; asynchronous on
    torch's current stream.  The scalar is not written."""
    _dev_call("ed25519_ScalarMult_dev" if clamp else "ed25519_ScalarMult_noclamp_dev", 2, (q, "q", 32), (ok, "ok", 1, _I32),
              (scalar, "scalar", 32), (point, "point", 32))


def ed25519_ScalarMultBase_dev(q, scalar, clamp=True):
    """Device form of ed25519_ScalarMultBase (clamp=False: _noclamp): scalar, q uint8[n, 32]; asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarMultBase_dev" if clamp else "ed25519_ScalarMultBase_noclamp_dev", 1, (q, "q", 32), (scalar, "scalar", 32))


def ed25519_PointAdd_dev(r, ok, p, q):
    """Device form of ed25519_PointAdd: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _dev_call("ed25519_PointAdd_dev", 2, (r, "r", 32), (ok, "ok", 1, _I32), (p, "p", 32), (q, "q", 32))


def ed25519_PointSub_dev(r, ok, p, q):
    """Device form of ed25519_PointSub: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _dev_call("ed25519_PointSub_dev", 2, (r, "r", 32), (ok, "ok", 1, _I32), (p, "p", 32), (q, "q", 32))


def ristretto255_IsValidPoint_dev(ok, point):
    """Device form of ristretto255_IsValidPoint: point uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _dev_call("ristretto255_IsValidPoint_dev", 1, (ok, "ok", 1, _I32), (point, "point", 32))


def ristretto255_FromHash_dev(p, hash):
    """Device form of ristretto255_FromHash: hash uint8[n, 64], p uint8[n, 32]; asynchronous on torch's current stream."""
    _dev_call("ristretto255_FromHash_dev", 1, (p, "p", 32), (hash, "hash", 64))


def ristretto255_ScalarMult_dev(q, ok, scalar, point):
    """Device form of ristretto255_ScalarMult: scalar, point, q uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream.
    The scalar is not written."""
    _dev_call("ristretto255_ScalarMult_dev", 2, (q, "q", 32), (ok, "ok", 1, _I32), (scalar, "scalar", 32), (point, "point", 32))


def ristretto255_ScalarMultBase_dev(q, scalar):
    """Device form of ristretto255_ScalarMultBase: scalar, q uint8[n, 32]; asynchronous on torch's current stream."""
    _dev_call("ristretto255_ScalarMultBase_dev", 1, (q, "q", 32), (scalar, "scalar", 32))


def ristretto255_PointAdd_dev(r, ok, p, q):
    """Device form of ristretto255_PointAdd: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _dev_call("ristretto255_PointAdd_dev", 2, (r, "r", 32), (ok, "ok", 1, _I32), (p, "p", 32), (q, "q", 32))


def ristretto255_PointSub_dev(r, ok, p, q):
    """Device form of ristretto255_PointSub: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _dev_call("ristretto255_PointSub_dev", 2, (r, "r", 32), (ok, "ok", 1, _I32), (p, "p", 32), (q, "q", 32))


def ed25519_ScalarReduce_dev(r, s):
    """Device form of ed25519_ScalarReduce: s uint8[n, 64], r uint8[n, 32]; asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarReduce_dev", 1, (r, "r", 32), (s, "s", 64))


def ed25519_ScalarAdd_dev(z, x, y):
    """Device form of ed25519_ScalarAdd: x, y, z uint8[n, 32] (z may be x or y); asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarAdd_dev", 1, (z, "z", 32), (x, "x", 32), (y, "y", 32))


def ed25519_ScalarSub_dev(z, x, y):
    """Device form of ed25519_ScalarSub: x, y, z uint8[n, 32] (z may be x or y); asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarSub_dev", 1, (z, "z", 32), (x, "x", 32), (y, "y", 32))


def ed25519_ScalarMul_dev(z, x, y):
    """Device form of ed25519_ScalarMul: x, y, z uint8[n, 32] (z may be x or y); asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarMul_dev", 1, (z, "z", 32), (x, "x", 32), (y, "y", 32))


def ed25519_ScalarNegate_dev(r, s):
    """Device form of ed25519_ScalarNegate: s, r uint8[n, 32] (r may be s); asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarNegate_dev", 1, (r, "r", 32), (s, "s", 32))


def ed25519_ScalarComplement_dev(r, s):
    """Device form of ed25519_ScalarComplement: s, r uint8[n, 32] (r may be s); asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarComplement_dev", 1, (r, "r", 32), (s, "s", 32))


def ed25519_ScalarMulAdd_dev(r, a, b, c):
    """Device form of ed25519_ScalarMulAdd: a, b, c, r uint8[n, 32] (r may be one of them); asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarMulAdd_dev", 1, (r, "r", 32), (a, "a", 32), (b, "b", 32), (c, "c", 32))


def ed25519_ScalarInvert_dev(recip, ok, s):
    """Device form of ed25519_ScalarInvert: s, recip uint8[n, 32] (recip may be s), ok int32[n, 1]; asynchronous on torch's current
    stream."""
    _dev_call("ed25519_ScalarInvert_dev", 2, (recip, "recip", 32), (ok, "ok", 1, _I32), (s, "s", 32))


def ed25519_ScalarIsCanonical_dev(ok, s):
    """Device form of ed25519_ScalarIsCanonical: s uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _dev_call("ed25519_ScalarIsCanonical_dev", 1, (ok, "ok", 1, _I32), (s, "s", 32))


def _h2c_call_dev(name, out, msg, dst, *extra):
    """out: the output's (tensor, name, width) as _dev_call takes it"""
    dst = bytes(dst)
    _dev_call(name, 1, out, (msg, "msg", _SIZED), dst, len(dst), *extra)


def c25519_ExpandMessageXmd_dev(out, msg, dst):
    """Device form of c25519_ExpandMessageXmd: msg uint8[n, msg_size], out uint8[n, len_in_bytes], dst bytes on the host;
    asynchronous on torch's current stream."""
    len_in_bytes = out.shape[1] if len(getattr(out, "shape", ())) == 2 else 0          # (anything else: `out` is refused below)
    _h2c_call_dev("c25519_ExpandMessageXmd_dev", (out, "out", None), msg, dst, len_in_bytes)


def ed25519_MapToCurve_dev(p, u):
    """Device form of ed25519_MapToCurve: u, p uint8[n, 32]; asynchronous on torch's current stream."""
    _dev_call("ed25519_MapToCurve_dev", 1, (p, "p", 32), (u, "u", 32))


def ed25519_HashToCurve_dev(p, msg, dst):
    """Device form of ed25519_HashToCurve: msg uint8[n, msg_size], p uint8[n, 32], dst bytes on the host; asynchronous on torch's
    current stream."""
    _h2c_call_dev("ed25519_HashToCurve_dev", (p, "p", 32), msg, dst)


def ed25519_EncodeToCurve_dev(p, msg, dst):
    """Device form of ed25519_EncodeToCurve: msg uint8[n, msg_size], p uint8[n, 32], dst bytes on the host."""
    _h2c_call_dev("ed25519_EncodeToCurve_dev", (p, "p", 32), msg, dst)


def ristretto255_HashToGroup_dev(p, msg, dst):
    """Device form of ristretto255_HashToGroup: msg uint8[n, msg_size], p uint8[n, 32], dst bytes on the host."""
    _h2c_call_dev("ristretto255_HashToGroup_dev", (p, "p", 32), msg, dst)


def ed25519_HashToScalar_dev(s, msg, dst):
    """Device form of ed25519_HashToScalar: msg uint8[n, msg_size], s uint8[n, 32], dst bytes on the host."""
    _h2c_call_dev("ed25519_HashToScalar_dev", (s, "s", 32), msg, dst)


def ed25519_VRF_Prove_dev(proof, priv, alpha):
    """Device form of ed25519_VRF_Prove: priv uint8[n, 64], alpha uint8[n, alpha_size], proof uint8[n, 80]; asynchronous on torch's
    current stream."""
    _dev_call("ed25519_VRF_Prove_dev", 1, (proof, "proof", 80), (priv, "priv", 64), (alpha, "alpha", _SIZED))


def ed25519_VRF_Verify_dev(beta, ok, pk, proof, alpha):
    """Device form of ed25519_VRF_Verify: pk uint8[n, 32], proof uint8[n, 80], alpha uint8[n, alpha_size], beta uint8[n, 64],
    ok int32[n, 1]; asynchronous on torch's current stream."""
    _dev_call("ed25519_VRF_Verify_dev", 2, (beta, "beta", 64), (ok, "ok", 1, _I32), (pk, "pk", 32), (proof, "proof", 80),
              (alpha, "alpha", _SIZED))


def ed25519_VRF_ProofToHash_dev(beta, ok, proof):
    """Device form of ed25519_VRF_ProofToHash: proof uint8[n, 80], beta uint8[n, 64], ok int32[n, 1]; asynchronous on torch's current
    stream."""
    _dev_call("ed25519_VRF_ProofToHash_dev", 2, (beta, "beta", 64), (ok, "ok", 1, _I32), (proof, "proof", 80))


def ed25519_SignMessage_dev(sig, priv, msg):
    _dev_call("ed25519_SignMessage_dev", 1, (sig, "sig", 64), (priv, "priv", 64), (msg, "msg", _SIZED))


def ed25519_Sign_Init_dev(ctx, priv):
    """Device form of ed25519_Sign_Init: priv uint8[n, 64], ctx uint8[n, 128]; asynchronous on torch's current stream."""
    _dev_call("ed25519_Sign_Init_dev", 1, (ctx, "ctx", SIGN_CTX_SIZE), (priv, "priv", 64))


def ed25519_SignMessage_indexed_dev(sig, ctxs, idx, msg):
    """Device form of ed25519_SignMessage_indexed: ctxs uint8[n_ctx, 128], idx int32[n, 1] (read as uint32), msg uint8[n, msg_size],
    sig uint8[n, 64].  An index >= n_ctx gives 64 zero bytes (nothing is checked on the host); does not synchronise."""
    _dev_call("ed25519_SignMessage_indexed_dev", 3, (sig, "sig", 64), (ctxs, "ctxs", SIGN_CTX_SIZE, _U8, _COUNTED), (idx, "idx", 1, _I32),
              (msg, "msg", _SIZED))


def ed25519_Verify_Check_indexed_dev(verdict, ctxs, idx, sig, msg, zip215=False):
    """Device form of ed25519_Verify_Check_indexed: ctxs uint8[n_ctx, 2080], idx int32[n, 1] (read as uint32), verdict int32[n, 1].
    An index >= n_ctx gives verdict 0 (nothing is checked on the host)."""
    _dev_call("ed25519_Verify_Check_zip215_indexed_dev" if zip215 else "ed25519_Verify_Check_indexed_dev", 3, (verdict, "verdict", 1, _I32),
              (ctxs, "ctxs", 2080, _U8, _COUNTED), (idx, "idx", 1, _I32), (sig, "sig", 64), (msg, "msg", _SIZED))


def ed25519_Verify_Check_zip215_indexed_dev(verdict, ctxs, idx, sig, msg):
    """Device form of ed25519_Verify_Check_zip215_indexed (same tensors as ed25519_Verify_Check_indexed_dev)."""
    ed25519_Verify_Check_indexed_dev(verdict, ctxs, idx, sig, msg, zip215=True)


def ed25519_Verify_Check_zip215_indexed_ragged_dev(verdict, ctxs, idx, sig, flat, offsets):
    """Device form with ragged messages: flat uint8[total, 1] message bytes, offsets int64[n + 1, 1] (read as uint64)."""
    _dev_call("ed25519_Verify_Check_zip215_indexed_ragged_dev", 3, (verdict, "verdict", 1, _I32), (ctxs, "ctxs", 2080, _U8, _COUNTED),
              (idx, "idx", 1, _I32), (sig, "sig", 64), (flat, "flat", 1, _U8, None), (offsets, "offsets", 1, _I64, "n+1"))


def ed25519_Verify_Check_dev(verdict, ctx, sig, msg, rules="plain"):
    """Device form of ed25519_Verify_Check (rules: "plain", "strict", "zip215"): ctx uint8[1, 2080] on the device, verdict int32[n, 1]."""
    _dev_call(f"ed25519_Verify_Check_{_RULES[rules]}dev", 2, (verdict, "verdict", 1, _I32), (ctx, "ctx", 2080, _U8, 1), (sig, "sig", 64),
              (msg, "msg", _SIZED))


def ed25519_Verify_Check_zip215_dev(verdict, ctx, sig, msg):
    """Device form of ed25519_Verify_Check_zip215: ctx uint8[1, 2080] on the device, verdict int32[n, 1]."""
    ed25519_Verify_Check_dev(verdict, ctx, sig, msg, "zip215")


def _verify_dev(verdict, sig, pk, msg, rules):
    _dev_call(f"ed25519_VerifySignature_{_RULES[rules]}dev", 1, (verdict, "verdict", 1, _I32), (sig, "sig", 64), (pk, "pk", 32),
              (msg, "msg", _SIZED))


def ed25519_VerifySignature_dev(verdict, sig, pk, msg, strict=False):
    _verify_dev(verdict, sig, pk, msg, "strict" if strict else "plain")


def ed25519_VerifySignature_strict_dev(verdict, sig, pk, msg):
    """Device form of ed25519_VerifySignature_strict: verdict int32[n, 1]."""
    _verify_dev(verdict, sig, pk, msg, "strict")


def ed25519_VerifySignature_zip215_dev(verdict, sig, pk, msg):
    """Device form of ed25519_VerifySignature_zip215: verdict int32[n, 1]."""
    _verify_dev(verdict, sig, pk, msg, "zip215")


def ed25519_VerifyBatch_zip215_dev(result, sig, pk, msg, seed):
    """Device form of ed25519_VerifyBatch_zip215: result int32[1, 1]; seed: 32 bytes of HOST memory (required); does not synchronise."""
    _dev_call("ed25519_VerifyBatch_zip215_dev", 1, (result, "result", 1, _I32, 1), (sig, "sig", 64), (pk, "pk", 32), (msg, "msg", _SIZED),
              after=(_seed(seed),))


def ed25519_VerifyBatch_zip215_ragged_dev(result, sig, pk, flat, offsets, seed):
    """Device form with ragged messages: flat uint8[total, 1] message bytes, offsets int64[n + 1, 1] (read as uint64)."""
    _dev_call("ed25519_VerifyBatch_zip215_ragged_dev", 1, (result, "result", 1, _I32, 1), (sig, "sig", 64), (pk, "pk", 32),
              (flat, "flat", 1, _U8, None), (offsets, "offsets", 1, _I64, "n+1"), after=(_seed(seed),))


def verify_batch_point_dev(out, sig, pk, msg, seed):
    """Test hook (c25519_amd_verify_batch_point_dev): out uint8[1, 32] <- enc(T) of the batch equation's point, always by the
    equation's kernels."""
    _dev_call("c25519_amd_verify_batch_point_dev", 1, (out, "out", 32, _U8, 1), (sig, "sig", 64), (pk, "pk", 32), (msg, "msg", _SIZED),
              after=(_seed(seed),))


def ed25519_VerifyBatch_zip215_indexed_dev(result, keys, idx, sig, msg, seed):
    """Device form of ed25519_VerifyBatch_zip215_indexed: keys uint8[n_key, 32], idx int32[n, 1] (read as uint32), result int32[1, 1];
    seed: 32 bytes of HOST memory (required).  An index >= n_key gives result 0 (nothing is checked on the host); does not synchronise."""
    _dev_call("ed25519_VerifyBatch_zip215_indexed_dev", 3, (result, "result", 1, _I32, 1), (keys, "keys", 32, _U8, _COUNTED),
              (idx, "idx", 1, _I32), (sig, "sig", 64), (msg, "msg", _SIZED), after=(_seed(seed),))


def ed25519_VerifyBatch_zip215_indexed_ragged_dev(result, keys, idx, sig, flat, offsets, seed):
    """Device form with ragged messages: flat uint8[total, 1] message bytes, offsets int64[n + 1, 1] (read as uint64)."""
    _dev_call("ed25519_VerifyBatch_zip215_indexed_ragged_dev", 3, (result, "result", 1, _I32, 1), (keys, "keys", 32, _U8, _COUNTED),
              (idx, "idx", 1, _I32), (sig, "sig", 64), (flat, "flat", 1, _U8, None), (offsets, "offsets", 1, _I64, "n+1"),
              after=(_seed(seed),))


def verify_batch_indexed_point_dev(out, keys, idx, sig, msg, seed):
    """Test hook (c25519_amd_verify_batch_indexed_point_dev): out uint8[1, 32] <- enc(T) of the COALESCED equation's point, always by the
    equation's kernels."""
    _dev_call("c25519_amd_verify_batch_indexed_point_dev", 3, (out, "out", 32, _U8, 1), (keys, "keys", 32, _U8, _COUNTED),
              (idx, "idx", 1, _I32), (sig, "sig", 64), (msg, "msg", _SIZED), after=(_seed(seed),))


def ed25519_Verify_Check_strict_dev(verdict, ctx, sig, msg):
    """Device form of ed25519_Verify_Check_strict: ctx uint8[1, 2080] on the device, verdict int32[n, 1]."""
    ed25519_Verify_Check_dev(verdict, ctx, sig, msg, "strict")
