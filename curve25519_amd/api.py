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

def curve25519_dh_CreateSharedKey(pk, sk):
    """n x curve25519_dh_CreateSharedKey.  Returns (shared, clamped_sk); inputs are not modified
    (the C function clamps in place -- the clamped copy is returned instead)."""
    pk = _np(pk, 32, "pk")
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    if pk.shape[0] != sk.shape[0]:
        raise ValueError("pk and sk must have the same number of rows")
    out = np.empty_like(pk)
    L = _lib.load()
    _lib.check(L.curve25519_dh_CreateSharedKey_batch(_ptr(out), _ptr(pk), _ptr(sk), pk.shape[0]),
               "curve25519_dh_CreateSharedKey_batch")
    return out, sk


def curve25519_dh_CreateSharedKey_one_peer(pk, sk):
    """n x curve25519_dh_CreateSharedKey with ONE peer key `pk` (32 bytes) for every secret.  Returns (shared, clamped_sk);
    the same bytes as curve25519_dh_CreateSharedKey with pk repeated n times (a large call walks a comb built for the peer)."""
    pk = _np(pk, 32, "pk")
    if pk.shape[0] != 1:
        raise ValueError("pk must be ONE 32-byte key")
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    out = np.empty_like(sk)
    _lib.check(_lib.load().curve25519_dh_CreateSharedKey_one_peer_batch(_ptr(out), _ptr(pk), _ptr(sk), sk.shape[0]),
               "curve25519_dh_CreateSharedKey_one_peer_batch")
    return out, sk


PEER_CTX_SIZE = 1600


def curve25519_dh_Peer_Init(pk):
    """n x curve25519_dh_Peer_Init: peer contexts, uint8[n, 1600] (pk || eligibility || 16 affine rows of 8 * pk's point)."""
    pk = _np(pk, 32, "pk")
    ctx = np.empty((pk.shape[0], PEER_CTX_SIZE), np.uint8)
    _lib.check(_lib.load().curve25519_dh_Peer_Init_batch(_ptr(ctx), _ptr(pk), pk.shape[0]), "curve25519_dh_Peer_Init_batch")
    return ctx


def curve25519_dh_CreateSharedKey_indexed(ctxs, idx, sk):
    """Many peers in one call: uint8[n_ctx, 1600] contexts (Peer_Init's), uint32[n] indices, n secrets -> (shared, clamped_sk),
    element i against the key of context idx[i] as curve25519_dh_CreateSharedKey would.  An index >= n_ctx raises EngineError."""
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    n = sk.shape[0]
    ctxs, idx = _ctx_index(ctxs, idx, n, PEER_CTX_SIZE, "secret")
    out = np.empty_like(sk)
    _lib.check(_lib.load().curve25519_dh_CreateSharedKey_indexed_batch(_ptr(out), _ptr(ctxs), ctxs.shape[0], _ptr(idx), _ptr(sk), n),
               "curve25519_dh_CreateSharedKey_indexed_batch")
    return out, sk


def x25519_indexed_last_ladder_elements():
    """elements of the calling thread's last CreateSharedKey_indexed call that ran the ladder (-1: no such call); synchronises"""
    return int(_lib.load().c25519_amd_x25519_indexed_last_ladder_elements())


def curve25519_dh_CalculatePublicKey(sk, fast=False):
    """n x curve25519_dh_CalculatePublicKey (or _fast).  Returns (pk, clamped_sk)."""
    sk = np.array(_np(sk, 32, "sk"), copy=True)
    out = np.empty_like(sk)
    L = _lib.load()
    fn = L.curve25519_dh_CalculatePublicKey_fast_batch if fast else L.curve25519_dh_CalculatePublicKey_batch
    _lib.check(fn(_ptr(out), _ptr(sk), sk.shape[0]), "curve25519_dh_CalculatePublicKey_batch")
    return out, sk


def ed25519_CreateKeyPair(sk):
    """n x ed25519_CreateKeyPair(blinding=NULL).  Returns (pub[n,32], priv[n,64])."""
    sk = _np(sk, 32, "sk")
    n = sk.shape[0]
    pub = np.empty((n, 32), np.uint8)
    priv = np.empty((n, 64), np.uint8)
    _lib.check(_lib.load().ed25519_CreateKeyPair_batch(_ptr(pub), _ptr(priv), _ptr(sk), n), "ed25519_CreateKeyPair_batch")
    return pub, priv


KEY_DECODES, KEY_CANONICAL, KEY_SMALL_ORDER, KEY_TORSION_FREE = 1, 2, 4, 8


def ed25519_ClassifyKey(pk):
    """n x ed25519_ClassifyKey: uint32[n] flags, the OR of KEY_DECODES, KEY_CANONICAL, KEY_SMALL_ORDER and KEY_TORSION_FREE
    (include/curve25519_amd.h states the rule; libsodium's "valid point" is flags == 11)."""
    pk = _np(pk, 32, "pk")
    flags = np.empty(pk.shape[0], np.uint32)
    _lib.check(_lib.load().ed25519_ClassifyKey_batch(_ptr(flags), _ptr(pk), pk.shape[0]), "ed25519_ClassifyKey_batch")
    return flags


def ed25519_PublicKey_to_X25519(pk):
    """n x ed25519_PublicKey_to_X25519.  Returns (xpk uint8[n, 32], ok int32[n]): ok = 1 and u = (1 + y) / (1 - y) for a key that
    decodes, is not of small order and is torsion-free; ok = 0 and 32 zero bytes for any other."""
    pk = _np(pk, 32, "pk")
    n = pk.shape[0]
    xpk = np.empty((n, 32), np.uint8)
    ok = np.empty(n, np.int32)
    _lib.check(_lib.load().ed25519_PublicKey_to_X25519_batch(_ptr(xpk), _ptr(ok), _ptr(pk), n), "ed25519_PublicKey_to_X25519_batch")
    return xpk, ok


def ed25519_PrivateKey_to_X25519(priv):
    """n x ed25519_PrivateKey_to_X25519: priv uint8[n, 64] (seed || pk) -> uint8[n, 32], the clamped first half of SHA-512(seed)."""
    priv = _np(priv, 64, "priv")
    xsk = np.empty((priv.shape[0], 32), np.uint8)
    _lib.check(_lib.load().ed25519_PrivateKey_to_X25519_batch(_ptr(xsk), _ptr(priv), priv.shape[0]),
               "ed25519_PrivateKey_to_X25519_batch")
    return xsk


def _group_pairs(a, b, names):
    a, b = _np(a, 32, names[0]), _np(b, 32, names[1])
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{names[0]} and {names[1]} must have the same number of rows")
    return a, b


def ed25519_ScalarMult(scalar, point, clamp=True):
    """n x ed25519_ScalarMult (clamp=False: ed25519_ScalarMult_noclamp).  Returns (q uint8[n, 32], ok int32[n]): ok = 1 and
    q = enc([e]P) where the point bytes decode (the ZIP-215 rule), ok = 0 and 32 zero bytes where they do not; e is the scalar
    clamped on a copy, or its low 255 bits.  The scalar is not modified."""
    scalar, point = _group_pairs(scalar, point, ("scalar", "point"))
    n = scalar.shape[0]
    q, ok = np.empty((n, 32), np.uint8), np.empty(n, np.int32)
    L = _lib.load()
    fn = L.ed25519_ScalarMult_batch if clamp else L.ed25519_ScalarMult_noclamp_batch
    _lib.check(fn(_ptr(q), _ptr(ok), _ptr(scalar), _ptr(point), n), "ed25519_ScalarMult_batch")
    return q, ok


def ed25519_ScalarMultBase(scalar, clamp=True):
    """n x ed25519_ScalarMultBase (clamp=False: ed25519_ScalarMultBase_noclamp): uint8[n, 32], enc([e]B) for every scalar."""
    scalar = _np(scalar, 32, "scalar")
    q = np.empty((scalar.shape[0], 32), np.uint8)
    L = _lib.load()
    fn = L.ed25519_ScalarMultBase_batch if clamp else L.ed25519_ScalarMultBase_noclamp_batch
    _lib.check(fn(_ptr(q), _ptr(scalar), scalar.shape[0]), "ed25519_ScalarMultBase_batch")
    return q


def _point_add(p, q, sub):
    p, q = _group_pairs(p, q, ("p", "q"))
    n = p.shape[0]
    r, ok = np.empty((n, 32), np.uint8), np.empty(n, np.int32)
    L = _lib.load()
    fn = L.ed25519_PointSub_batch if sub else L.ed25519_PointAdd_batch
    _lib.check(fn(_ptr(r), _ptr(ok), _ptr(p), _ptr(q), n), "ed25519_PointSub_batch" if sub else "ed25519_PointAdd_batch")
    return r, ok


def ed25519_PointAdd(p, q):
    """n x ed25519_PointAdd.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = enc(P + Q) where both decode, else zeros."""
    return _point_add(p, q, False)


def ed25519_PointSub(p, q):
    """n x ed25519_PointSub.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = enc(P - Q) where both decode, else zeros."""
    return _point_add(p, q, True)


def ristretto255_IsValidPoint(point):
    """n x ristretto255_IsValidPoint: int32[n], 1 where the 32 bytes decode by RFC 9496 section 4.3.1."""
    point = _np(point, 32, "point")
    ok = np.empty(point.shape[0], np.int32)
    _lib.check(_lib.load().ristretto255_IsValidPoint_batch(_ptr(ok), _ptr(point), point.shape[0]), "ristretto255_IsValidPoint_batch")
    return ok


def ristretto255_FromHash(hash):
    """n x ristretto255_FromHash: hash uint8[n, 64] -> uint8[n, 32], ENCODE(MAP(low half) + MAP(high half))."""
    hash = _np(hash, 64, "hash")
    p = np.empty((hash.shape[0], 32), np.uint8)
    _lib.check(_lib.load().ristretto255_FromHash_batch(_ptr(p), _ptr(hash), hash.shape[0]), "ristretto255_FromHash_batch")
    return p


def ristretto255_ScalarMult(scalar, point):
    """n x ristretto255_ScalarMult.  Returns (q uint8[n, 32], ok int32[n]): ok = 1 and q = ENCODE([e]P) where the point bytes decode
    (the identity is 32 zero bytes with ok = 1), ok = 0 and 32 zero bytes where they do not; e is the scalar's low 255 bits.  The
    scalar is not modified."""
    scalar, point = _group_pairs(scalar, point, ("scalar", "point"))
    n = scalar.shape[0]
    q, ok = np.empty((n, 32), np.uint8), np.empty(n, np.int32)
    _lib.check(_lib.load().ristretto255_ScalarMult_batch(_ptr(q), _ptr(ok), _ptr(scalar), _ptr(point), n), "ristretto255_ScalarMult_batch")
    return q, ok


def ristretto255_ScalarMultBase(scalar):
    """n x ristretto255_ScalarMultBase: uint8[n, 32], ENCODE([e]B) for every scalar."""
    scalar = _np(scalar, 32, "scalar")
    q = np.empty((scalar.shape[0], 32), np.uint8)
    _lib.check(_lib.load().ristretto255_ScalarMultBase_batch(_ptr(q), _ptr(scalar), scalar.shape[0]), "ristretto255_ScalarMultBase_batch")
    return q


def _rist_point_add(p, q, sub):
    p, q = _group_pairs(p, q, ("p", "q"))
    n = p.shape[0]
    r, ok = np.empty((n, 32), np.uint8), np.empty(n, np.int32)
    L = _lib.load()
    fn = L.ristretto255_PointSub_batch if sub else L.ristretto255_PointAdd_batch
    _lib.check(fn(_ptr(r), _ptr(ok), _ptr(p), _ptr(q), n), "ristretto255_PointSub_batch" if sub else "ristretto255_PointAdd_batch")
    return r, ok


def ristretto255_PointAdd(p, q):
    """n x ristretto255_PointAdd.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = ENCODE(P + Q) where both decode, else zeros."""
    return _rist_point_add(p, q, False)


def ristretto255_PointSub(p, q):
    """n x ristretto255_PointSub.  Returns (r uint8[n, 32], ok int32[n]): ok = 1 and r = ENCODE(P - Q) where both decode, else zeros."""
    return _rist_point_add(p, q, True)


def _scalar_rows(arrays, names, width=32):
    arrays = [_np(a, width, name) for a, name in zip(arrays, names)]
    if any(a.shape[0] != arrays[0].shape[0] for a in arrays):
        raise ValueError(f"{', '.join(names)} must have the same number of rows")
    return arrays


def _scalar_call(name, arrays, names, width=32):
    arrays = _scalar_rows(arrays, names, width)
    n = arrays[0].shape[0]
    r = np.empty((n, 32), np.uint8)
    _lib.check(getattr(_lib.load(), name)(_ptr(r), *[_ptr(a) for a in arrays], n), name)
    return r


def ed25519_ScalarReduce(s):
    """n x ed25519_ScalarReduce: s uint8[n, 64] -> uint8[n, 32], the 512-bit value mod L."""
    return _scalar_call("ed25519_ScalarReduce_batch", (s,), ("s",), 64)


def ed25519_ScalarAdd(x, y):
    """n x ed25519_ScalarAdd: uint8[n, 32], x + y mod L (canonical; the inputs may be any 32-byte values)."""
    return _scalar_call("ed25519_ScalarAdd_batch", (x, y), ("x", "y"))


def ed25519_ScalarSub(x, y):
    """n x ed25519_ScalarSub: uint8[n, 32], x - y mod L."""
    return _scalar_call("ed25519_ScalarSub_batch", (x, y), ("x", "y"))


def ed25519_ScalarMul(x, y):
    """n x ed25519_ScalarMul: uint8[n, 32], x y mod L."""
    return _scalar_call("ed25519_ScalarMul_batch", (x, y), ("x", "y"))


def ed25519_ScalarNegate(s):
    """n x ed25519_ScalarNegate: uint8[n, 32], -s mod L."""
    return _scalar_call("ed25519_ScalarNegate_batch", (s,), ("s",))


def ed25519_ScalarComplement(s):
    """n x ed25519_ScalarComplement: uint8[n, 32], 1 - s mod L."""
    return _scalar_call("ed25519_ScalarComplement_batch", (s,), ("s",))


def ed25519_ScalarMulAdd(a, b, c):
    """n x ed25519_ScalarMulAdd: uint8[n, 32], a b + c mod L."""
    return _scalar_call("ed25519_ScalarMulAdd_batch", (a, b, c), ("a", "b", "c"))


def ed25519_ScalarInvert(s):
    """n x ed25519_ScalarInvert.  Returns (recip uint8[n, 32], ok int32[n]): ok = 1 and recip = 1 / s mod L where s mod L != 0, ok = 0
    and 32 zero bytes where it is zero (s = L included: zero is judged after reduction)."""
    s = _np(s, 32, "s")
    n = s.shape[0]
    recip, ok = np.empty((n, 32), np.uint8), np.empty(n, np.int32)
    _lib.check(_lib.load().ed25519_ScalarInvert_batch(_ptr(recip), _ptr(ok), _ptr(s), n), "ed25519_ScalarInvert_batch")
    return recip, ok


def ed25519_ScalarIsCanonical(s):
    """n x ed25519_ScalarIsCanonical: int32[n], 1 where the 32 bytes are below L."""
    s = _np(s, 32, "s")
    ok = np.empty(s.shape[0], np.int32)
    _lib.check(_lib.load().ed25519_ScalarIsCanonical_batch(_ptr(ok), _ptr(s), s.shape[0]), "ed25519_ScalarIsCanonical_batch")
    return ok


def _h2c_args(msg, dst):
    """(msg uint8[n, msg_size], dst as a bytes buffer): the rows of a hashing call and its domain separation tag"""
    msg = np.ascontiguousarray(msg, dtype=np.uint8)
    if msg.ndim != 2:
        raise ValueError(f"msg must have shape (n, msg_size), got {msg.shape}")
    return msg, bytes(dst)


def _h2c_call(name, msg, dst):
    msg, dst = _h2c_args(msg, dst)
    n, msg_size = msg.shape
    out = np.empty((n, 32), np.uint8)
    _lib.check(getattr(_lib.load(), name)(_ptr(out), _ptr(msg) if msg_size else None, msg_size, dst, len(dst), n), name)
    return out


def c25519_ExpandMessageXmd(msg, dst, len_in_bytes):
    """n x expand_message_xmd over SHA-512 (RFC 9380 section 5.3.1): msg uint8[n, msg_size], dst 1 .. 255 bytes ->
    uint8[n, len_in_bytes], 1 <= len_in_bytes <= 16320."""
    msg, dst = _h2c_args(msg, dst)
    n, msg_size = msg.shape
    out = np.empty((n, max(int(len_in_bytes), 0)), np.uint8)
    _lib.check(_lib.load().c25519_ExpandMessageXmd_batch(_ptr(out), _ptr(msg) if msg_size else None, msg_size, dst, len(dst),
                                                         int(len_in_bytes), n), "c25519_ExpandMessageXmd_batch")
    return out


def ed25519_MapToCurve(u):
    """n x map_to_curve_elligator2_edwards25519 (RFC 9380 section 6.8.2): u uint8[n, 32] (little-endian, bit 255 masked, mod p) ->
    the Ed25519 encodings uint8[n, 32]; no cofactor cleared, u = 0 gives the identity."""
    u = _np(u, 32, "u")
    p = np.empty((u.shape[0], 32), np.uint8)
    _lib.check(_lib.load().ed25519_MapToCurve_batch(_ptr(p), _ptr(u), u.shape[0]), "ed25519_MapToCurve_batch")
    return p


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
    n = priv.shape[0]
    alpha = _vrf_alpha(alpha, n)
    proof = np.empty((n, 80), np.uint8)
    _lib.check(_lib.load().ed25519_VRF_Prove_batch(_ptr(proof), _ptr(priv), _ptr(alpha) if alpha.shape[1] else None, alpha.shape[1], n),
               "ed25519_VRF_Prove_batch")
    return proof


def ed25519_VRF_Verify(pk, proof, alpha):
    """n x ECVRF verify with validate_key = TRUE (RFC 9381 section 5.3): pk uint8[n, 32], proof uint8[n, 80], alpha
    uint8[n, alpha_size].  Returns (beta uint8[n, 64], ok int32[n]): ok = 1 and the VRF output where the proof is valid, ok = 0 and
    64 zero bytes where it is not."""
    pk, proof = _np(pk, 32, "pk"), _np(proof, 80, "proof")
    n = pk.shape[0]
    if proof.shape[0] != n:
        raise ValueError("pk and proof must have the same number of rows")
    alpha = _vrf_alpha(alpha, n)
    beta, ok = np.empty((n, 64), np.uint8), np.empty(n, np.int32)
    _lib.check(_lib.load().ed25519_VRF_Verify_batch(_ptr(beta), _ptr(ok), _ptr(pk), _ptr(proof), _ptr(alpha) if alpha.shape[1] else None,
                                                    alpha.shape[1], n), "ed25519_VRF_Verify_batch")
    return beta, ok


def ed25519_VRF_ProofToHash(proof):
    """n x ECVRF proof_to_hash (RFC 9381 section 5.2): proof uint8[n, 80].  Returns (beta uint8[n, 64], ok int32[n]): ok = 0 and 64
    zero bytes where the proof does not decode.  The proof is NOT verified."""
    proof = _np(proof, 80, "proof")
    n = proof.shape[0]
    beta, ok = np.empty((n, 64), np.uint8), np.empty(n, np.int32)
    _lib.check(_lib.load().ed25519_VRF_ProofToHash_batch(_ptr(beta), _ptr(ok), _ptr(proof), n), "ed25519_VRF_ProofToHash_batch")
    return beta, ok


def ed25519_SignMessage(priv, msg):
    """n x ed25519_SignMessage(blinding=NULL) over fixed-length messages msg[n, msg_size]."""
    priv = _np(priv, 64, "priv")
    n = priv.shape[0]
    msg, msg_size = _msgs(msg, n)
    sig = np.empty((n, 64), np.uint8)
    _lib.check(_lib.load().ed25519_SignMessage_batch(_ptr(sig), _ptr(priv), _ptr(msg), msg_size, n), "ed25519_SignMessage_batch")
    return sig


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
    n = priv.shape[0]
    if len(messages) != n:
        raise ValueError("one message per private key")
    flat, offsets = _ragged(messages)
    sig = np.empty((n, 64), np.uint8)
    _lib.check(_lib.load().ed25519_SignMessage_ragged_batch(_ptr(sig), _ptr(priv), _ptr(flat), _ptr(offsets), n),
               "ed25519_SignMessage_ragged_batch")
    return sig


SIGN_CTX_SIZE = 128


def ed25519_Sign_Init(priv):
    """n x ed25519_Sign_Init: signer contexts, uint8[n, 128] (a || prefix || pk || 0).  As secret as the private keys."""
    priv = _np(priv, 64, "priv")
    ctx = np.empty((priv.shape[0], SIGN_CTX_SIZE), np.uint8)
    _lib.check(_lib.load().ed25519_Sign_Init_batch(_ptr(ctx), _ptr(priv), priv.shape[0]), "ed25519_Sign_Init_batch")
    return ctx


def ed25519_SignMessage_indexed(ctxs, idx, msg):
    """Many keys in one call: uint8[n_ctx, 128] contexts (Sign_Init's), uint32[n] indices, fixed-length messages msg[n, msg_size] ->
    uint8[n, 64], signature i as ed25519_SignMessage under the key of context idx[i].  An index >= n_ctx raises EngineError."""
    n = np.size(idx)
    ctxs, idx = _ctx_index(ctxs, idx, n, SIGN_CTX_SIZE, "message")
    msg, msg_size = _msgs(msg, n)
    sig = np.empty((n, 64), np.uint8)
    _lib.check(_lib.load().ed25519_SignMessage_indexed_batch(_ptr(sig), _ptr(ctxs), ctxs.shape[0], _ptr(idx), _ptr(msg), msg_size, n),
               "ed25519_SignMessage_indexed_batch")
    return sig


def ed25519_SignMessage_indexed_ragged(ctxs, idx, messages):
    """ed25519_SignMessage_indexed with per-element message lengths (`messages`: sequence of bytes-like)."""
    n = len(messages)
    ctxs, idx = _ctx_index(ctxs, idx, n, SIGN_CTX_SIZE, "message")
    flat, offsets = _ragged(messages)
    sig = np.empty((n, 64), np.uint8)
    _lib.check(_lib.load().ed25519_SignMessage_indexed_ragged_batch(_ptr(sig), _ptr(ctxs), ctxs.shape[0], _ptr(idx), _ptr(flat),
                                                                     _ptr(offsets), n), "ed25519_SignMessage_indexed_ragged_batch")
    return sig


# the verification rule sets (include/curve25519_amd.h): what goes between "ed25519_VerifySignature_" and the form's suffix
_RULES = {"plain": "", "strict": "strict_", "zip215": "zip215_"}


def _verify_ragged(sig, pk, messages, rules):
    sig = _np(sig, 64, "sig")
    pk = _np(pk, 32, "pk")
    n = sig.shape[0]
    if len(messages) != n or pk.shape[0] != n:
        raise ValueError("one message and one key per signature")
    flat, offsets = _ragged(messages)
    ok = np.empty(n, np.int32)
    name = f"ed25519_VerifySignature_{_RULES[rules]}ragged_batch"
    _lib.check(getattr(_lib.load(), name)(_ptr(ok), _ptr(sig), _ptr(pk), _ptr(flat), _ptr(offsets), n), name)
    return ok


def ed25519_VerifySignature_ragged(sig, pk, messages, strict=False):
    return _verify_ragged(sig, pk, messages, "strict" if strict else "plain")


def ed25519_VerifySignature_strict_ragged(sig, pk, messages):
    """ed25519_VerifySignature_strict with per-element message lengths (`messages`: sequence of bytes-like)."""
    return _verify_ragged(sig, pk, messages, "strict")


def _verify(sig, pk, msg, rules):
    sig = _np(sig, 64, "sig")
    pk = _np(pk, 32, "pk")
    n = sig.shape[0]
    if pk.shape[0] != n:
        raise ValueError("sig and pk must have the same number of rows")
    msg, msg_size = _msgs(msg, n)
    ok = np.empty(n, np.int32)
    name = f"ed25519_VerifySignature_{_RULES[rules]}batch"
    _lib.check(getattr(_lib.load(), name)(_ptr(ok), _ptr(sig), _ptr(pk), _ptr(msg), msg_size, n), name)
    return ok


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
    pk = _np(pk, 32, "pk")
    ctx = np.empty((pk.shape[0], 2080), np.uint8)
    _lib.check(_lib.load().ed25519_Verify_Init_batch(_ptr(ctx), _ptr(pk), pk.shape[0]), "ed25519_Verify_Init_batch")
    return ctx


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
    n = sig.shape[0]
    msg, msg_size = _msgs(msg, n)
    ok = np.empty(n, np.int32)
    name = f"ed25519_Verify_Check_{_RULES[rules or ('strict' if strict else 'plain')]}batch"
    _lib.check(getattr(_lib.load(), name)(_ptr(ok), _ptr(ctx), _ptr(sig), _ptr(msg), msg_size, n), name)
    return ok


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
    n = sig.shape[0]
    ctxs, idx = _ctx_index(ctxs, idx, n)
    msg, msg_size = _msgs(msg, n)
    ok = np.empty(n, np.int32)
    name = "ed25519_Verify_Check_zip215_indexed_batch" if zip215 else "ed25519_Verify_Check_indexed_batch"
    _lib.check(getattr(_lib.load(), name)(_ptr(ok), _ptr(ctxs), ctxs.shape[0], _ptr(idx), _ptr(sig), _ptr(msg), msg_size, n), name)
    return ok


def ed25519_Verify_Check_indexed_ragged(ctxs, idx, sig, messages, zip215=False):
    """ed25519_Verify_Check_indexed with per-element message lengths (`messages`: sequence of bytes-like)."""
    sig = _np(sig, 64, "sig")
    n = sig.shape[0]
    ctxs, idx = _ctx_index(ctxs, idx, n)
    if len(messages) != n:
        raise ValueError("one message per signature")
    flat, offsets = _ragged(messages)
    ok = np.empty(n, np.int32)
    name = "ed25519_Verify_Check_zip215_indexed_ragged_batch" if zip215 else "ed25519_Verify_Check_indexed_ragged_batch"
    _lib.check(getattr(_lib.load(), name)(_ptr(ok), _ptr(ctxs), ctxs.shape[0], _ptr(idx), _ptr(sig), _ptr(flat), _ptr(offsets), n), name)
    return ok


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

def _check(t, width, name, n=None, dtype=None, device=None):
    import torch
    dtype = torch.uint8 if dtype is None else dtype
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor")
    if t.dim() != 2 or (width is not None and t.shape[1] != width):
        raise ValueError(f"{name} must have shape (n, {width}), got {tuple(t.shape)}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name} must have {n} rows like the other arguments, got {t.shape[0]}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, the other arguments on {device}")
    return C.c_void_p(t.data_ptr())


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
    n, d = pk.shape[0], pk.device
    args = (_check(shared, 32, "shared", n, device=d), _check(pk, 32, "pk"), _check(sk, 32, "sk", n, device=d))
    with _on(pk) as st:
        _lib.check(_lib.load().curve25519_dh_CreateSharedKey_dev(*args, n, st), "curve25519_dh_CreateSharedKey_dev")


def curve25519_dh_CreateSharedKey_one_peer_dev(shared, pk, sk):
    """In-place device form with ONE peer key (`pk`: a (1, 32) or (32,) uint8 CUDA tensor): writes `shared`, clamps `sk`;
    asynchronous on torch's current stream (the comb-or-ladder decision is taken on the device)."""
    n, d = sk.shape[0], sk.device
    pk = pk.reshape(1, -1) if getattr(pk, "dim", lambda: 2)() == 1 else pk
    args = (_check(shared, 32, "shared", n, device=d), _check(pk, 32, "pk", 1, device=d),
            _check(sk, 32, "sk"))
    with _on(sk) as st:
        _lib.check(_lib.load().curve25519_dh_CreateSharedKey_one_peer_dev(*args, n, st), "curve25519_dh_CreateSharedKey_one_peer_dev")


def curve25519_dh_Peer_Init_dev(ctx, pk):
    """Device form of curve25519_dh_Peer_Init: pk uint8[n, 32], ctx uint8[n, 1600]; asynchronous on torch's current stream."""
    n, d = pk.shape[0], pk.device
    args = (_check(ctx, PEER_CTX_SIZE, "ctx", n, device=d), _check(pk, 32, "pk"))
    with _on(pk) as st:
        _lib.check(_lib.load().curve25519_dh_Peer_Init_dev(*args, n, st), "curve25519_dh_Peer_Init_dev")


def curve25519_dh_CreateSharedKey_indexed_dev(shared, ctxs, idx, sk):
    """Device form of curve25519_dh_CreateSharedKey_indexed: ctxs uint8[n_ctx, 1600], idx int32[n, 1] (read as uint32), writes
    `shared`, clamps `sk`.  An index >= n_ctx gives 32 zero bytes (nothing is checked on the host); does not synchronise."""
    import torch
    n, d = sk.shape[0], sk.device
    args = (_check(shared, 32, "shared", n, device=d), _check(ctxs, PEER_CTX_SIZE, "ctxs", device=d), ctxs.shape[0],
            _check(idx, 1, "idx", n, dtype=torch.int32, device=d), _check(sk, 32, "sk"))
    with _on(sk) as st:
        _lib.check(_lib.load().curve25519_dh_CreateSharedKey_indexed_dev(*args, n, st), "curve25519_dh_CreateSharedKey_indexed_dev")


def curve25519_dh_CalculatePublicKey_dev(pk, sk, fast=False):
    L = _lib.load()
    fn = L.curve25519_dh_CalculatePublicKey_fast_dev if fast else L.curve25519_dh_CalculatePublicKey_dev
    n, d = sk.shape[0], sk.device
    args = (_check(pk, 32, "pk", n, device=d), _check(sk, 32, "sk"))
    with _on(sk) as st:
        _lib.check(fn(*args, n, st), "curve25519_dh_CalculatePublicKey_dev")


def ed25519_CreateKeyPair_dev(pub, priv, sk):
    n, d = sk.shape[0], sk.device
    args = (_check(pub, 32, "pub", n, device=d), _check(priv, 64, "priv", n, device=d), _check(sk, 32, "sk"))
    with _on(sk) as st:
        _lib.check(_lib.load().ed25519_CreateKeyPair_dev(*args, n, st), "ed25519_CreateKeyPair_dev")


def ed25519_ClassifyKey_dev(flags, pk):
    """Device form of ed25519_ClassifyKey: pk uint8[n, 32], flags int32[n, 1] (read as uint32); asynchronous on torch's current stream."""
    import torch
    n, d = pk.shape[0], pk.device
    args = (_check(flags, 1, "flags", n, dtype=torch.int32, device=d), _check(pk, 32, "pk"))
    with _on(pk) as st:
        _lib.check(_lib.load().ed25519_ClassifyKey_dev(*args, n, st), "ed25519_ClassifyKey_dev")


def ed25519_PublicKey_to_X25519_dev(xpk, ok, pk):
    """Device form of ed25519_PublicKey_to_X25519: pk uint8[n, 32], xpk uint8[n, 32], ok int32[n, 1]; asynchronous on torch's
    current stream."""
    import torch
    n, d = pk.shape[0], pk.device
    args = (_check(xpk, 32, "xpk", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(pk, 32, "pk"))
    with _on(pk) as st:
        _lib.check(_lib.load().ed25519_PublicKey_to_X25519_dev(*args, n, st), "ed25519_PublicKey_to_X25519_dev")


def ed25519_PrivateKey_to_X25519_dev(xsk, priv):
    """Device form of ed25519_PrivateKey_to_X25519: priv uint8[n, 64], xsk uint8[n, 32]; asynchronous on torch's current stream."""
    n, d = priv.shape[0], priv.device
    args = (_check(xsk, 32, "xsk", n, device=d), _check(priv, 64, "priv"))
    with _on(priv) as st:
        _lib.check(_lib.load().ed25519_PrivateKey_to_X25519_dev(*args, n, st), "ed25519_PrivateKey_to_X25519_dev")


def ed25519_ScalarMult_dev(q, ok, scalar, point, clamp=True):
    """Device form of ed25519_ScalarMult (clamp=False: _noclamp): scalar, point, q uint8[n, 32], ok int32[n, 1]; asynchronous on
    torch's current stream.  The scalar is not written."""
    import torch
    L = _lib.load()
    fn = L.ed25519_ScalarMult_dev if clamp else L.ed25519_ScalarMult_noclamp_dev
    n, d = scalar.shape[0], scalar.device
    args = (_check(q, 32, "q", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(scalar, 32, "scalar"),
            _check(point, 32, "point", n, device=d))
    with _on(scalar) as st:
        _lib.check(fn(*args, n, st), "ed25519_ScalarMult_dev")


def ed25519_ScalarMultBase_dev(q, scalar, clamp=True):
    """Device form of ed25519_ScalarMultBase (clamp=False: _noclamp): scalar, q uint8[n, 32]; asynchronous on torch's current stream."""
    L = _lib.load()
    fn = L.ed25519_ScalarMultBase_dev if clamp else L.ed25519_ScalarMultBase_noclamp_dev
    n, d = scalar.shape[0], scalar.device
    args = (_check(q, 32, "q", n, device=d), _check(scalar, 32, "scalar"))
    with _on(scalar) as st:
        _lib.check(fn(*args, n, st), "ed25519_ScalarMultBase_dev")


def _point_add_dev(r, ok, p, q, sub):
    import torch
    L = _lib.load()
    fn = L.ed25519_PointSub_dev if sub else L.ed25519_PointAdd_dev
    n, d = p.shape[0], p.device
    args = (_check(r, 32, "r", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(p, 32, "p"),
            _check(q, 32, "q", n, device=d))
    with _on(p) as st:
        _lib.check(fn(*args, n, st), "ed25519_PointSub_dev" if sub else "ed25519_PointAdd_dev")


def ed25519_PointAdd_dev(r, ok, p, q):
    """Device form of ed25519_PointAdd: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _point_add_dev(r, ok, p, q, False)


def ed25519_PointSub_dev(r, ok, p, q):
    """Device form of ed25519_PointSub: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _point_add_dev(r, ok, p, q, True)


def ristretto255_IsValidPoint_dev(ok, point):
    """Device form of ristretto255_IsValidPoint: point uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    import torch
    n, d = point.shape[0], point.device
    args = (_check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(point, 32, "point"))
    with _on(point) as st:
        _lib.check(_lib.load().ristretto255_IsValidPoint_dev(*args, n, st), "ristretto255_IsValidPoint_dev")


def ristretto255_FromHash_dev(p, hash):
    """Device form of ristretto255_FromHash: hash uint8[n, 64], p uint8[n, 32]; asynchronous on torch's current stream."""
    n, d = hash.shape[0], hash.device
    args = (_check(p, 32, "p", n, device=d), _check(hash, 64, "hash"))
    with _on(hash) as st:
        _lib.check(_lib.load().ristretto255_FromHash_dev(*args, n, st), "ristretto255_FromHash_dev")


def ristretto255_ScalarMult_dev(q, ok, scalar, point):
    """Device form of ristretto255_ScalarMult: scalar, point, q uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream.
    The scalar is not written."""
    import torch
    n, d = scalar.shape[0], scalar.device
    args = (_check(q, 32, "q", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(scalar, 32, "scalar"),
            _check(point, 32, "point", n, device=d))
    with _on(scalar) as st:
        _lib.check(_lib.load().ristretto255_ScalarMult_dev(*args, n, st), "ristretto255_ScalarMult_dev")


def ristretto255_ScalarMultBase_dev(q, scalar):
    """Device form of ristretto255_ScalarMultBase: scalar, q uint8[n, 32]; asynchronous on torch's current stream."""
    n, d = scalar.shape[0], scalar.device
    args = (_check(q, 32, "q", n, device=d), _check(scalar, 32, "scalar"))
    with _on(scalar) as st:
        _lib.check(_lib.load().ristretto255_ScalarMultBase_dev(*args, n, st), "ristretto255_ScalarMultBase_dev")


def _rist_point_add_dev(r, ok, p, q, sub):
    import torch
    L = _lib.load()
    fn = L.ristretto255_PointSub_dev if sub else L.ristretto255_PointAdd_dev
    n, d = p.shape[0], p.device
    args = (_check(r, 32, "r", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(p, 32, "p"),
            _check(q, 32, "q", n, device=d))
    with _on(p) as st:
        _lib.check(fn(*args, n, st), "ristretto255_PointSub_dev" if sub else "ristretto255_PointAdd_dev")


def ristretto255_PointAdd_dev(r, ok, p, q):
    """Device form of ristretto255_PointAdd: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _rist_point_add_dev(r, ok, p, q, False)


def ristretto255_PointSub_dev(r, ok, p, q):
    """Device form of ristretto255_PointSub: p, q, r uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    _rist_point_add_dev(r, ok, p, q, True)


def _scalar_call_dev(name, r, inputs, names, width=32):
    n, d = inputs[0].shape[0], inputs[0].device
    args = [_check(r, 32, "r", n, device=d)] + [_check(t, width, nm, n, device=d) for t, nm in zip(inputs, names)]
    with _on(inputs[0]) as st:
        _lib.check(getattr(_lib.load(), name)(*args, n, st), name)


def ed25519_ScalarReduce_dev(r, s):
    """Device form of ed25519_ScalarReduce: s uint8[n, 64], r uint8[n, 32]; asynchronous on torch's current stream."""
    _scalar_call_dev("ed25519_ScalarReduce_dev", r, (s,), ("s",), 64)


def ed25519_ScalarAdd_dev(z, x, y):
    """Device form of ed25519_ScalarAdd: x, y, z uint8[n, 32] (z may be x or y); asynchronous on torch's current stream."""
    _scalar_call_dev("ed25519_ScalarAdd_dev", z, (x, y), ("x", "y"))


def ed25519_ScalarSub_dev(z, x, y):
    """Device form of ed25519_ScalarSub: x, y, z uint8[n, 32] (z may be x or y); asynchronous on torch's current stream."""
    _scalar_call_dev("ed25519_ScalarSub_dev", z, (x, y), ("x", "y"))


def ed25519_ScalarMul_dev(z, x, y):
    """Device form of ed25519_ScalarMul: x, y, z uint8[n, 32] (z may be x or y); asynchronous on torch's current stream."""
    _scalar_call_dev("ed25519_ScalarMul_dev", z, (x, y), ("x", "y"))


def ed25519_ScalarNegate_dev(r, s):
    """Device form of ed25519_ScalarNegate: s, r uint8[n, 32] (r may be s); asynchronous on torch's current stream."""
    _scalar_call_dev("ed25519_ScalarNegate_dev", r, (s,), ("s",))


def ed25519_ScalarComplement_dev(r, s):
    """Device form of ed25519_ScalarComplement: s, r uint8[n, 32] (r may be s); asynchronous on torch's current stream."""
    _scalar_call_dev("ed25519_ScalarComplement_dev", r, (s,), ("s",))


def ed25519_ScalarMulAdd_dev(r, a, b, c):
    """Device form of ed25519_ScalarMulAdd: a, b, c, r uint8[n, 32] (r may be one of them); asynchronous on torch's current stream."""
    _scalar_call_dev("ed25519_ScalarMulAdd_dev", r, (a, b, c), ("a", "b", "c"))


def ed25519_ScalarInvert_dev(recip, ok, s):
    """Device form of ed25519_ScalarInvert: s, recip uint8[n, 32] (recip may be s), ok int32[n, 1]; asynchronous on torch's current
    stream."""
    import torch
    n, d = s.shape[0], s.device
    args = (_check(recip, 32, "recip", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(s, 32, "s"))
    with _on(s) as st:
        _lib.check(_lib.load().ed25519_ScalarInvert_dev(*args, n, st), "ed25519_ScalarInvert_dev")


def ed25519_ScalarIsCanonical_dev(ok, s):
    """Device form of ed25519_ScalarIsCanonical: s uint8[n, 32], ok int32[n, 1]; asynchronous on torch's current stream."""
    import torch
    n, d = s.shape[0], s.device
    args = (_check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(s, 32, "s"))
    with _on(s) as st:
        _lib.check(_lib.load().ed25519_ScalarIsCanonical_dev(*args, n, st), "ed25519_ScalarIsCanonical_dev")


def _h2c_call_dev(name, out, width, msg, dst, *extra):
    n, d = msg.shape[0], msg.device
    dst = bytes(dst)
    args = (_check(out, width, "out", n, device=d), _check(msg, None, "msg") if msg.shape[1] else None)
    with _on(msg) as st:
        _lib.check(getattr(_lib.load(), name)(*args, msg.shape[1], dst, len(dst), *extra, n, st), name)


def c25519_ExpandMessageXmd_dev(out, msg, dst):
    """Device form of c25519_ExpandMessageXmd: msg uint8[n, msg_size], out uint8[n, len_in_bytes], dst bytes on the host;
    asynchronous on torch's current stream."""
    _h2c_call_dev("c25519_ExpandMessageXmd_dev", out, None, msg, dst, out.shape[1])


def ed25519_MapToCurve_dev(p, u):
    """Device form of ed25519_MapToCurve: u, p uint8[n, 32]; asynchronous on torch's current stream."""
    n, d = u.shape[0], u.device
    args = (_check(p, 32, "p", n, device=d), _check(u, 32, "u"))
    with _on(u) as st:
        _lib.check(_lib.load().ed25519_MapToCurve_dev(*args, n, st), "ed25519_MapToCurve_dev")


def ed25519_HashToCurve_dev(p, msg, dst):
    """Device form of ed25519_HashToCurve: msg uint8[n, msg_size], p uint8[n, 32], dst bytes on the host; asynchronous on torch's
    current stream."""
    _h2c_call_dev("ed25519_HashToCurve_dev", p, 32, msg, dst)


def ed25519_EncodeToCurve_dev(p, msg, dst):
    """Device form of ed25519_EncodeToCurve: msg uint8[n, msg_size], p uint8[n, 32], dst bytes on the host."""
    _h2c_call_dev("ed25519_EncodeToCurve_dev", p, 32, msg, dst)


def ristretto255_HashToGroup_dev(p, msg, dst):
    """Device form of ristretto255_HashToGroup: msg uint8[n, msg_size], p uint8[n, 32], dst bytes on the host."""
    _h2c_call_dev("ristretto255_HashToGroup_dev", p, 32, msg, dst)


def ed25519_HashToScalar_dev(s, msg, dst):
    """Device form of ed25519_HashToScalar: msg uint8[n, msg_size], s uint8[n, 32], dst bytes on the host."""
    _h2c_call_dev("ed25519_HashToScalar_dev", s, 32, msg, dst)


def ed25519_VRF_Prove_dev(proof, priv, alpha):
    """Device form of ed25519_VRF_Prove: priv uint8[n, 64], alpha uint8[n, alpha_size], proof uint8[n, 80]; asynchronous on torch's
    current stream."""
    n, d = priv.shape[0], priv.device
    args = (_check(proof, 80, "proof", n, device=d), _check(priv, 64, "priv"),
            _check(alpha, None, "alpha", n, device=d) if alpha.shape[1] else None)
    with _on(priv) as st:
        _lib.check(_lib.load().ed25519_VRF_Prove_dev(*args, alpha.shape[1], n, st), "ed25519_VRF_Prove_dev")


def ed25519_VRF_Verify_dev(beta, ok, pk, proof, alpha):
    """Device form of ed25519_VRF_Verify: pk uint8[n, 32], proof uint8[n, 80], alpha uint8[n, alpha_size], beta uint8[n, 64],
    ok int32[n, 1]; asynchronous on torch's current stream."""
    import torch
    n, d = pk.shape[0], pk.device
    args = (_check(beta, 64, "beta", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(pk, 32, "pk"),
            _check(proof, 80, "proof", n, device=d), _check(alpha, None, "alpha", n, device=d) if alpha.shape[1] else None)
    with _on(pk) as st:
        _lib.check(_lib.load().ed25519_VRF_Verify_dev(*args, alpha.shape[1], n, st), "ed25519_VRF_Verify_dev")


def ed25519_VRF_ProofToHash_dev(beta, ok, proof):
    """Device form of ed25519_VRF_ProofToHash: proof uint8[n, 80], beta uint8[n, 64], ok int32[n, 1]; asynchronous on torch's current
    stream."""
    import torch
    n, d = proof.shape[0], proof.device
    args = (_check(beta, 64, "beta", n, device=d), _check(ok, 1, "ok", n, dtype=torch.int32, device=d), _check(proof, 80, "proof"))
    with _on(proof) as st:
        _lib.check(_lib.load().ed25519_VRF_ProofToHash_dev(*args, n, st), "ed25519_VRF_ProofToHash_dev")


def ed25519_SignMessage_dev(sig, priv, msg):
    n, d = priv.shape[0], priv.device
    args = (_check(sig, 64, "sig", n, device=d), _check(priv, 64, "priv"), _check(msg, None, "msg", n, device=d))
    with _on(priv) as st:
        _lib.check(_lib.load().ed25519_SignMessage_dev(*args, msg.shape[1], n, st), "ed25519_SignMessage_dev")


def ed25519_Sign_Init_dev(ctx, priv):
    """Device form of ed25519_Sign_Init: priv uint8[n, 64], ctx uint8[n, 128]; asynchronous on torch's current stream."""
    n, d = priv.shape[0], priv.device
    args = (_check(ctx, SIGN_CTX_SIZE, "ctx", n, device=d), _check(priv, 64, "priv"))
    with _on(priv) as st:
        _lib.check(_lib.load().ed25519_Sign_Init_dev(*args, n, st), "ed25519_Sign_Init_dev")


def ed25519_SignMessage_indexed_dev(sig, ctxs, idx, msg):
    """Device form of ed25519_SignMessage_indexed: ctxs uint8[n_ctx, 128], idx int32[n, 1] (read as uint32), msg uint8[n, msg_size],
    sig uint8[n, 64].  An index >= n_ctx gives 64 zero bytes (nothing is checked on the host); does not synchronise."""
    import torch
    n, d = msg.shape[0], msg.device
    args = (_check(sig, 64, "sig", n, device=d), _check(ctxs, SIGN_CTX_SIZE, "ctxs", device=d), ctxs.shape[0],
            _check(idx, 1, "idx", n, dtype=torch.int32, device=d), _check(msg, None, "msg", n, device=d))
    with _on(msg) as st:
        _lib.check(_lib.load().ed25519_SignMessage_indexed_dev(*args, msg.shape[1], n, st), "ed25519_SignMessage_indexed_dev")


def ed25519_Verify_Check_indexed_dev(verdict, ctxs, idx, sig, msg, zip215=False):
    """Device form of ed25519_Verify_Check_indexed: ctxs uint8[n_ctx, 2080], idx int32[n, 1] (read as uint32), verdict int32[n, 1].
    An index >= n_ctx gives verdict 0 (nothing is checked on the host)."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(verdict, 1, "verdict", n, dtype=torch.int32, device=d), _check(ctxs, 2080, "ctxs", device=d))
    args += (ctxs.shape[0], _check(idx, 1, "idx", n, dtype=torch.int32, device=d), _check(sig, 64, "sig"),
             _check(msg, None, "msg", n, device=d))
    name = "ed25519_Verify_Check_zip215_indexed_dev" if zip215 else "ed25519_Verify_Check_indexed_dev"
    with _on(sig) as st:
        _lib.check(getattr(_lib.load(), name)(*args, msg.shape[1], n, st), name)


def ed25519_Verify_Check_zip215_indexed_dev(verdict, ctxs, idx, sig, msg):
    """Device form of ed25519_Verify_Check_zip215_indexed (same tensors as ed25519_Verify_Check_indexed_dev)."""
    ed25519_Verify_Check_indexed_dev(verdict, ctxs, idx, sig, msg, zip215=True)


def ed25519_Verify_Check_zip215_indexed_ragged_dev(verdict, ctxs, idx, sig, flat, offsets):
    """Device form with ragged messages: flat uint8[total, 1] message bytes, offsets int64[n + 1, 1] (read as uint64)."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(verdict, 1, "verdict", n, dtype=torch.int32, device=d), _check(ctxs, 2080, "ctxs", device=d), ctxs.shape[0],
            _check(idx, 1, "idx", n, dtype=torch.int32, device=d), _check(sig, 64, "sig"), _check(flat, 1, "flat", device=d),
            _check(offsets, 1, "offsets", n + 1, dtype=torch.int64, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().ed25519_Verify_Check_zip215_indexed_ragged_dev(*args, n, st), "ed25519_Verify_Check_zip215_indexed_ragged_dev")


def ed25519_Verify_Check_dev(verdict, ctx, sig, msg, rules="plain"):
    """Device form of ed25519_Verify_Check (rules: "plain", "strict", "zip215"): ctx uint8[1, 2080] on the device, verdict int32[n, 1]."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(verdict, 1, "verdict", n, dtype=torch.int32, device=d), _check(ctx, 2080, "ctx", 1, device=d), _check(sig, 64, "sig"),
            _check(msg, None, "msg", n, device=d))
    name = f"ed25519_Verify_Check_{_RULES[rules]}dev"
    with _on(sig) as st:
        _lib.check(getattr(_lib.load(), name)(*args, msg.shape[1], n, st), name)


def ed25519_Verify_Check_zip215_dev(verdict, ctx, sig, msg):
    """Device form of ed25519_Verify_Check_zip215: ctx uint8[1, 2080] on the device, verdict int32[n, 1]."""
    ed25519_Verify_Check_dev(verdict, ctx, sig, msg, "zip215")


def _verify_dev(verdict, sig, pk, msg, rules):
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(verdict, 1, "verdict", n, dtype=torch.int32, device=d), _check(sig, 64, "sig"),
            _check(pk, 32, "pk", n, device=d), _check(msg, None, "msg", n, device=d))
    name = f"ed25519_VerifySignature_{_RULES[rules]}dev"
    with _on(sig) as st:
        _lib.check(getattr(_lib.load(), name)(*args, msg.shape[1], n, st), name)


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
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(result, 1, "result", 1, dtype=torch.int32, device=d), _check(sig, 64, "sig"), _check(pk, 32, "pk", n, device=d),
            _check(msg, None, "msg", n, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().ed25519_VerifyBatch_zip215_dev(*args, msg.shape[1], n, _seed(seed), st), "ed25519_VerifyBatch_zip215_dev")


def ed25519_VerifyBatch_zip215_ragged_dev(result, sig, pk, flat, offsets, seed):
    """Device form with ragged messages: flat uint8[total, 1] message bytes, offsets int64[n + 1, 1] (read as uint64)."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(result, 1, "result", 1, dtype=torch.int32, device=d), _check(sig, 64, "sig"), _check(pk, 32, "pk", n, device=d),
            _check(flat, 1, "flat", device=d), _check(offsets, 1, "offsets", n + 1, dtype=torch.int64, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().ed25519_VerifyBatch_zip215_ragged_dev(*args, n, _seed(seed), st), "ed25519_VerifyBatch_zip215_ragged_dev")


def verify_batch_point_dev(out, sig, pk, msg, seed):
    """Test hook (c25519_amd_verify_batch_point_dev): out uint8[1, 32] <- enc(T) of the batch equation's point, always by the
    equation's kernels."""
    n, d = sig.shape[0], sig.device
    args = (_check(out, 32, "out", 1, device=d), _check(sig, 64, "sig"), _check(pk, 32, "pk", n, device=d), _check(msg, None, "msg", n, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().c25519_amd_verify_batch_point_dev(*args, msg.shape[1], n, _seed(seed), st), "c25519_amd_verify_batch_point_dev")


def ed25519_VerifyBatch_zip215_indexed_dev(result, keys, idx, sig, msg, seed):
    """Device form of ed25519_VerifyBatch_zip215_indexed: keys uint8[n_key, 32], idx int32[n, 1] (read as uint32), result int32[1, 1];
    seed: 32 bytes of HOST memory (required).  An index >= n_key gives result 0 (nothing is checked on the host); does not synchronise."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(result, 1, "result", 1, dtype=torch.int32, device=d), _check(keys, 32, "keys", device=d), keys.shape[0],
            _check(idx, 1, "idx", n, dtype=torch.int32, device=d), _check(sig, 64, "sig"), _check(msg, None, "msg", n, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().ed25519_VerifyBatch_zip215_indexed_dev(*args, msg.shape[1], n, _seed(seed), st),
                   "ed25519_VerifyBatch_zip215_indexed_dev")


def ed25519_VerifyBatch_zip215_indexed_ragged_dev(result, keys, idx, sig, flat, offsets, seed):
    """Device form with ragged messages: flat uint8[total, 1] message bytes, offsets int64[n + 1, 1] (read as uint64)."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(result, 1, "result", 1, dtype=torch.int32, device=d), _check(keys, 32, "keys", device=d), keys.shape[0],
            _check(idx, 1, "idx", n, dtype=torch.int32, device=d), _check(sig, 64, "sig"), _check(flat, 1, "flat", device=d),
            _check(offsets, 1, "offsets", n + 1, dtype=torch.int64, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().ed25519_VerifyBatch_zip215_indexed_ragged_dev(*args, n, _seed(seed), st),
                   "ed25519_VerifyBatch_zip215_indexed_ragged_dev")


def verify_batch_indexed_point_dev(out, keys, idx, sig, msg, seed):
    """Test hook (c25519_amd_verify_batch_indexed_point_dev): out uint8[1, 32] <- enc(T) of the COALESCED equation's point, always by the
    equation's kernels."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(out, 32, "out", 1, device=d), _check(keys, 32, "keys", device=d), keys.shape[0],
            _check(idx, 1, "idx", n, dtype=torch.int32, device=d), _check(sig, 64, "sig"), _check(msg, None, "msg", n, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().c25519_amd_verify_batch_indexed_point_dev(*args, msg.shape[1], n, _seed(seed), st),
                   "c25519_amd_verify_batch_indexed_point_dev")


def ed25519_Verify_Check_strict_dev(verdict, ctx, sig, msg):
    """Device form of ed25519_Verify_Check_strict: ctx uint8[1, 2080] on the device, verdict int32[n, 1]."""
    import torch
    n, d = sig.shape[0], sig.device
    args = (_check(verdict, 1, "verdict", n, dtype=torch.int32, device=d), _check(ctx, 2080, "ctx", 1, device=d), _check(sig, 64, "sig"),
            _check(msg, None, "msg", n, device=d))
    with _on(sig) as st:
        _lib.check(_lib.load().ed25519_Verify_Check_strict_dev(*args, msg.shape[1], n, st), "ed25519_Verify_Check_strict_dev")
