"""The ZIP-215 batch equation with COALESCED KEYS (include/curve25519_amd.h, above ed25519_VerifyBatch_zip215_indexed_dev) in Python big
integers, on top of tests/batch_eq_model.py: the expected result and the expected point of the test hook
c25519_amd_verify_batch_indexed_point_dev for the CPU emulator and the GPU tests.  Element i's key is keys[idx[i]]; the terms of one
key are merged: T = [sum z_i S_i mod L]B - sum_i [z_i]R_i - sum_j [(sum_{i: idx[i] = j} z_i k_i) mod L]A_j."""
import hashlib

import numpy as np

import batch_eq_model as bm
from vectors import ED_B, L
from zip215_cases import zip215_decode


def _challenges(seed, n, index):
    return bm.challenges(seed, n) if index is None else [bm.challenge(bytes(seed), int(i)) for i in index]


def key_sums(keys, idx, sig, msg, seed, index=None):
    """(sums, s_sum, left_out): sums[j] = the integer sum of a_i = z_i k_i mod L over the elements that name key j and stay in the
    equation ({j: sum}, only the keys with such an element); s_sum = sum z_i S_i mod L over them; left_out[i]: element i is rejected
    (S >= L, an R or a named key that does not decode, an index out of range).  index: as in batch_point"""
    n, n_key = len(sig), len(keys)
    z = _challenges(seed, n, index)
    sums, s_sum, left_out = {}, 0, [False] * n
    decoded = {}
    for i in range(n):
        j, sg, m = int(idx[i]), bytes(sig[i]), bytes(msg[i])
        S = int.from_bytes(sg[32:], "little")
        if j < n_key and j not in decoded:
            decoded[j] = zip215_decode(bytes(keys[j]))
        if S >= L or j >= n_key or decoded[j] is None or zip215_decode(sg[:32]) is None:
            left_out[i] = True
            continue
        k = int.from_bytes(hashlib.sha512(sg[:32] + bytes(keys[j]) + m).digest(), "little") % L
        sums[j] = sums.get(j, 0) + z[i] * k % L
        s_sum = (s_sum + z[i] * S) % L
    return sums, s_sum, left_out


def batch_point(keys, idx, sig, msg, seed, index=None):
    """(T, ok): the coalesced point in affine coordinates over the elements that stay, ok = every element stayed.  A key that no
    remaining element names is never decoded.  index: the elements' own indices in the call (default 0 .. n - 1): the rows are then a
    subset of a batch, and T is that subset's share of the batch's point provided no row outside the subset names one of its keys.
    The elements that share one R (byte for byte) are taken together, [sum z_i]R with the sum as an integer: the same point whatever
    R's order."""
    sums, s_sum, left_out = key_sums(keys, idx, sig, msg, seed, index)
    z = _challenges(seed, len(sig), index)
    acc = bm._mul(s_sum, bm._ext(ED_B))
    z_of_r = {}
    for i in range(len(sig)):
        if not left_out[i]:
            r = bytes(sig[i][:32])
            z_of_r[r] = z_of_r.get(r, 0) + z[i]
    for r, total in z_of_r.items():
        acc = bm._add(acc, bm._neg(bm._mul(total, bm._ext(zip215_decode(r)))))
    for j, total in sums.items():
        if total % L:
            acc = bm._add(acc, bm._neg(bm._mul(total % L, bm._ext(zip215_decode(bytes(keys[j]))))))
    return bm._affine(acc), not any(left_out)


def batch_result(keys, idx, sig, msg, seed):
    """the `result` of ed25519_VerifyBatch_zip215_indexed_* for one equation over the whole batch"""
    if len(sig) == 0:
        return 1
    T, ok = batch_point(keys, idx, sig, msg, seed)
    return int(ok and bm._affine(bm._mul(8, bm._ext(T))) == (0, 1))


def gathered_result(keys, idx, sig, msg, seed):
    """what the un-indexed call gives on the gathered keys (an index out of range: 0, as the *_dev forms answer)"""
    keys, idx = np.asarray(keys), np.asarray(idx, dtype=np.int64)
    if (idx >= len(keys)).any():
        return 0
    return bm.batch_result(sig, keys[idx], msg, seed)


def cancelling_pair_one_key(oracle, seed=0xBA7C4E1):
    """two honest signatures under ONE key with S_0 + 5 and S_1 - 5: (keys[1, 32], idx[2], sig, msg).  Both single verdicts are 0, and the
    pair's terms share one point of the coalesced equation."""
    pub, priv = oracle.ed25519_keypair(oracle.random_bytes((1, 32), seed))
    msg = oracle.random_bytes((2, 32), seed + 1)
    sig = oracle.ed25519_sign(np.repeat(priv, 2, axis=0), msg).copy()
    for i, delta in ((0, 5), (1, -5)):
        S = int.from_bytes(sig[i, 32:].tobytes(), "little") + delta
        assert 0 <= S < L
        sig[i, 32:] = np.frombuffer(S.to_bytes(32, "little"), np.uint8)
    return pub, np.zeros(2, np.uint32), sig, msg


def distinct_keys(pk):
    """(keys, idx) with keys[idx] == pk: the distinct rows of pk in order of first appearance"""
    seen, keys, idx = {}, [], np.zeros(len(pk), np.uint32)
    for i, row in enumerate(pk):
        b = bytes(row)
        if b not in seen:
            seen[b] = len(keys)
            keys.append(np.frombuffer(b, np.uint8))
        idx[i] = seen[b]
    return np.stack(keys), idx
