"""The ZIP-215 verification rule (include/curve25519_amd.h, above ed25519_VerifySignature_zip215_batch) in Python big integers, and the
edge set the CPU and GPU tests of the ZIP-215 calls share.  Unlike tests/strict_cases.py this model decides the whole verdict, the
group equation included: the reference has no such rule, so nothing here comes from it."""
import functools
import hashlib

import numpy as np

import strict_cases as sc
from vectors import L, P, ED_B, ed_add, ed_decode, ed_mul, degenerate_signature_cases, small_order_encodings, torsion_signature_cases

MASK255 = 2**255 - 1
NEUTRAL = (0, 1)
GRID_MSG = b"Zcash"


def _int(row):
    return int.from_bytes(bytes(row), "little")


def zip215_decode(enc):
    """the point of a 32-byte string, or None: y = the low 255 bits mod p, x = the square root with the parity of bit 255; x = 0 with
    the sign bit set decodes to x = 0 (ed_decode returns x = P there, unreduced)"""
    v = _int(enc)
    pt = ed_decode((v & MASK255) % P, v >> 255)
    return None if pt is None else (pt[0] % P, pt[1])


def zip215_verdict(sig, pk, msg):
    """rules 1-4 for one element (bytes-like each)"""
    return _verdict(bytes(sig), bytes(pk), bytes(msg))


@functools.lru_cache(maxsize=None)
def _verdict(sig, pk, msg):
    S = _int(sig[32:])
    if S >= L:
        return 0
    A, R = zip215_decode(pk), zip215_decode(sig[:32])
    if A is None or R is None:
        return 0
    k = int.from_bytes(hashlib.sha512(sig[:32] + pk + msg).digest(), "little") % L
    neg = lambda p: ((P - p[0]) % P, p[1])  # noqa: E731
    W = ed_add(ed_add(ed_mul(S, ED_B), neg(ed_mul(k, A))), neg(R))
    return int(ed_mul(8, W) == NEUTRAL)


def zip215_rule(sig, pk, msg):
    """int32[n] of verdicts; msg: uint8[n, len] or a sequence of bytes-like"""
    return np.array([zip215_verdict(sig[i], pk[i], msg[i]) for i in range(len(sig))], np.int32)


def _rows(rows):
    return np.stack([np.frombuffer(bytes(r), np.uint8) for r in rows])


def conformance_grid():
    """ZIP-215's own test set: every (key, R) pair of the 14 encodings of the 8 small-order points, S = 0, message b"Zcash": all valid.
    (sig[196, 64], pk[196, 32], msg[196, 5])"""
    encs = [e for e, _ in small_order_encodings()]
    sigs = [r + bytes(32) for _ in encs for r in encs]
    pks = [a for a in encs for _ in encs]
    return _rows(sigs), _rows(pks), _rows([GRID_MSG] * len(sigs))


def noncanonical_y_strings():
    """the 38 strings with y in [p, 2^255): 19 values, either sign bit.  uint8[38, 32]"""
    return _rows([(y | (s << 255)).to_bytes(32, "little") for y in range(P, 2**255) for s in (0, 1)])


def decode_inputs():
    """what the decoding test runs: the 38 non-canonical y strings, the 14 small-order encodings, x = 0 with the sign bit"""
    extra = [(1 | (1 << 255)).to_bytes(32, "little"), ((P - 1) | (1 << 255)).to_bytes(32, "little")]
    return np.concatenate([noncanonical_y_strings(), _rows([e for e, _ in small_order_encodings()]), _rows(extra)])


def edge_set(oracle, msg_len=32):
    """(sig, pk, msg[n, msg_len]): tests/strict_cases.py's edge_cases unchanged as inputs, the non-canonical y strings as R (verdict 0
    inputs: nobody knows a discrete logarithm for the ten that are not of small order), a sample of the conformance grid and of the
    degenerate set (8-byte messages there, so those two are re-keyed to msg_len by the model, not by their makers' expectations)"""
    sig, pk, msg = sc.edge_cases(oracle)
    assert msg.shape[1] == msg_len
    extra_sig = [bytes(r) + sig[0][32:].tobytes() for r in noncanonical_y_strings()]
    extra_pk = [pk[0].tobytes()] * len(extra_sig)
    extra_msg = [msg[0].tobytes()] * len(extra_sig)
    # small-order pairs under a msg_len-byte message: S = 0 is accepted whatever the residue, S = 1 never, S = L rejected by rule 1
    encs = [e for e, _ in small_order_encodings()]
    for i, a in enumerate(encs):
        r = encs[(5 * i + 3) % len(encs)]
        m = bytes([i]) * msg_len
        for S in (0, 1, L):
            extra_sig.append(r + S.to_bytes(32, "little"))
            extra_pk.append(a)
            extra_msg.append(m)
    return (np.concatenate([sig, _rows(extra_sig)]), np.concatenate([pk, _rows(extra_pk)]), np.concatenate([msg, _rows(extra_msg)]))


def degenerate():
    """tests/vectors.py's degenerate_signature_cases: (sig, pk, msg[n, 8], label)"""
    return degenerate_signature_cases()


def torsion():
    return torsion_signature_cases(count=3)
