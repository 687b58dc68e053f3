"""CPU tests of the ZIP-215 batch equation with coalesced keys (what ed25519_VerifyBatch_zip215_indexed_* runs on the device from
BATCH_EQ_INDEXED_MIN).  The lane-level device source, curve25519_amd/csrc/msm25519.cuh, is compiled by g++ against the C model of the
gfx950 primitives (tests/host_emul/verify_batch_indexed.cpp, tests/host_emul/build.py's build_lib); a host counting sort and host
accumulation stand in for the kernels' atomics.  Expected points and results: the rule in Python big integers
(tests/batch_eq_indexed_model.py), and the un-indexed rule on the gathered keys (tests/batch_eq_model.py) for the result."""
import ctypes as C
import random

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import batch_eq_indexed_model as im
import batch_eq_model as bm
import zip215_cases as zc
from vectors import L

vp, sz = C.c_void_p, C.c_size_t
WIDTHS = (8, 10, 13)
SEEDS = [bytes([19 * j + 5]) * 32 for j in range(8)]


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_keyeq_fold": [vp, vp, C.c_int], "emul_keyeq": [vp, vp, sz, vp, vp, vp, sz, sz, vp, C.c_int]},
                   "verify_batch_indexed.cpp", "libc25519_emul_verify_batch_indexed.so")
    yield lib
    assert_no_mad_overflow(lib)


def ptr(a):
    return a.ctypes.data_as(vp)


def run(lib, keys, idx, sig, msg, seed, c):
    """(enc(T), result) of the emulated chain"""
    keys, sig, msg = (np.ascontiguousarray(a, np.uint8) for a in (keys, sig, msg))
    idx = np.ascontiguousarray(idx, np.uint32)
    point = np.zeros(32, np.uint8)
    sd = np.frombuffer(seed, np.uint8).copy()
    res = lib.emul_keyeq(ptr(point), ptr(keys), len(keys), ptr(idx), ptr(sig), ptr(msg), msg.shape[1], len(sig), ptr(sd), c)
    return point, res


def honest(oracle, n, n_key, seed):
    """n honest signatures under n_key keys, element i under key i mod n_key: (keys, idx, sig, msg)"""
    pub, priv = oracle.ed25519_keypair(oracle.random_bytes((n_key, 32), seed))
    idx = (np.arange(n) % n_key).astype(np.uint32)
    msg = oracle.random_bytes((n, 32), seed + 1)
    return pub, idx, oracle.ed25519_sign(priv[idx], msg), msg


def concat(*cases):
    """several (keys, idx, sig, msg) as one batch, every case's indices moved behind the keys before it"""
    off, keys, idx, sig, msg = 0, [], [], [], []
    for k, i, s, m in cases:
        keys.append(k), idx.append(np.asarray(i, np.uint32) + off), sig.append(s), msg.append(m)
        off += len(k)
    return tuple(np.concatenate(a) for a in (keys, idx, sig, msg))


@pytest.fixture(scope="module")
def inputs(oracle):
    """the all-valid inputs: name -> (keys, idx, sig, msg[n, 32])"""
    out = {"one key": honest(oracle, 24, 1, 0xC0A1E5C0), "three keys": honest(oracle, 24, 3, 0xC0A1E5C2),
           "n keys": honest(oracle, 24, 24, 0xC0A1E5C4)}
    tsig, tpk, tmsg = zc.torsion()
    tkeys, tidx = im.distinct_keys(tpk)
    assert len(tsig) == 24 and len(tkeys) == 3
    out["torsion"] = tkeys, tidx, tsig, tmsg
    gsig, gpk, _ = (a[::7] for a in zc.conformance_grid())
    gkeys, gidx = im.distinct_keys(gpk)
    assert 1 < len(gkeys) < len(gpk)
    out["grid"] = gkeys, gidx, gsig, oracle.random_bytes((len(gsig), 32), 0xC0A1E5C6)   # S = 0 on small-order points: valid under any message
    keys, idx, sig, msg = concat(out["one key"], out["three keys"], out["torsion"], out["grid"])
    perm = np.random.default_rng(0xC0A1E5C7).permutation(len(sig))
    kperm = np.random.default_rng(0xC0A1E5C8).permutation(len(keys))                    # ... and the keys in another order
    inv = np.argsort(kperm).astype(np.uint32)
    out["mixed"] = keys[kperm], inv[idx][perm], sig[perm], msg[perm]
    for name, (keys, idx, sig, msg) in out.items():
        if name != "mixed":
            assert zc.zip215_rule(sig, keys[idx], msg).all(), name
    return out


NAMES = ["one key", "three keys", "n keys", "torsion", "grid", "mixed"]


# ---- the fold -------------------------------------------------------------------------------------------------------------

def _bias(c):
    return sum(1 << (w * c + c - 1) for w in range(-(-255 // c) - 1))


@pytest.mark.parametrize("c", range(7, 14))
def test_fold_of_the_word_sums_is_the_sum_mod_L(lib, c):
    """eight 64-bit sums of 32-bit words, as the kernels accumulate them -> sum a_i mod L, biased; with n <= 2^26 a sum stays below 2^58,
    and all eight at 2^58 - 1 is the largest input the fold can meet"""
    rnd = random.Random(0xF01D + c)
    cases = [[(1 << 58) - 1] * 8, [0] * 8, [1] + [0] * 7, [0] * 7 + [(1 << 58) - 1], [(1 << 58) - 1] + [0] * 7]
    cases += [[(L >> (32 * j)) & 0xffffffff for j in range(8)]]                   # the words of L itself: total 0 mod L
    cases += [[(2 * L >> (32 * j)) & 0xffffffff for j in range(8)]]
    for count in (1, 2, 1000, 1 << 26):                                           # `count` scalars below L, summed word by word
        for _ in range(6):
            words = [0] * 8
            total = 0
            for _ in range(min(count, 50)):
                a = rnd.getrandbits(256) % L
                rep = count // min(count, 50)
                total += a * rep
                for j in range(8):
                    words[j] += ((a >> (32 * j)) & 0xffffffff) * rep
            assert max(words) < 1 << 58
            cases.append(words)
    cases += [[rnd.getrandbits(58) for _ in range(8)] for _ in range(50)]
    out = np.zeros(32, np.uint8)
    for words in cases:
        total = sum(w << (32 * j) for j, w in enumerate(words))
        arr = np.array(words, np.uint64)
        nz = lib.emul_keyeq_fold(ptr(out), ptr(arr), c)
        assert int.from_bytes(out.tobytes(), "little") - _bias(c) == total % L, (c, words)
        assert nz == int(total % L != 0)


# ---- the chain against the model ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_point_and_result_equal_the_model(lib, inputs, name, c):
    keys, idx, sig, msg = inputs[name]
    want, ok = im.batch_point(keys, idx, sig, msg, SEEDS[0])
    got, res = run(lib, keys, idx, sig, msg, SEEDS[0], c)
    assert ok and np.array_equal(got, bm.encode(want)), (name, c)
    assert res == 1 == im.batch_result(keys, idx, sig, msg, SEEDS[0]) == im.gathered_result(keys, idx, sig, msg, SEEDS[0])


@pytest.mark.parametrize("name", NAMES)
def test_one_flipped_S_gives_zero(lib, inputs, name):
    keys, idx, sig, msg = inputs[name]
    bad = sig.copy()
    bad[len(bad) // 2, 40] ^= 0x04
    for j, seed in enumerate(SEEDS[1:4]):
        assert im.gathered_result(keys, idx, sig, msg, seed) == 1 == run(lib, keys, idx, sig, msg, seed, WIDTHS[j])[1], (name, j)
        assert im.batch_result(keys, idx, bad, msg, seed) == 0 == im.gathered_result(keys, idx, bad, msg, seed)
        assert run(lib, keys, idx, bad, msg, seed, WIDTHS[j])[1] == 0, (name, j)


def test_torsion_rows_three_times_the_points_differ_and_both_results_are_one(lib):
    """24 elements over 3 mixed-order keys, repeated three times: [a mod L]A != [a]A there, so the coalesced point differs from the
    un-indexed one by an 8-torsion point, and [8] removes the difference"""
    tsig, tpk, tmsg = (np.concatenate([a, a, a]) for a in zc.torsion())
    keys, idx = im.distinct_keys(tpk)
    assert len(keys) == 3
    coalesced, ok = im.batch_point(keys, idx, tsig, tmsg, SEEDS[4])
    plain, ok2 = bm.batch_point(tsig, tpk, tmsg, SEEDS[4])
    assert ok and ok2 and coalesced != plain
    diff = bm._add(bm._ext(coalesced), bm._neg(bm._ext(plain)))
    assert bm._affine(bm._mul(8, diff)) == (0, 1)
    for c in WIDTHS:
        got, res = run(lib, keys, idx, tsig, tmsg, SEEDS[4], c)
        assert np.array_equal(got, bm.encode(coalesced)) and res == 1 == bm.batch_result(tsig, tpk, tmsg, SEEDS[4])
    bad = tsig.copy()
    bad[31, 40] ^= 0x04
    assert bm.batch_result(bad, tpk, tmsg, SEEDS[4]) == 0 == run(lib, keys, idx, bad, tmsg, SEEDS[4], 10)[1]


def test_one_key_cancelling_pair_is_rejected_for_eight_seeds(lib, oracle):
    keys, idx, sig, msg = im.cancelling_pair_one_key(oracle)
    assert zc.zip215_rule(sig, keys[idx], msg).tolist() == [0, 0]
    for j, seed in enumerate(SEEDS):
        assert im.batch_result(keys, idx, sig, msg, seed) == 0 == im.gathered_result(keys, idx, sig, msg, seed)
        assert run(lib, keys, idx, sig, msg, seed, WIDTHS[j % 3])[1] == 0, j


def test_an_unnamed_undecodable_key_is_not_part_of_the_batch(lib, oracle):
    keys, idx, sig, msg = honest(oracle, 9, 3, 0xC0A1E5D0)
    keys = np.concatenate([keys[:1], bm.undecodable()[None], keys[1:], bm.undecodable()[None]])
    idx = np.where(idx >= 1, idx + 1, idx).astype(np.uint32)
    want, ok = im.batch_point(keys, idx, sig, msg, SEEDS[5])
    assert ok and im.gathered_result(keys, idx, sig, msg, SEEDS[5]) == 1
    for c in WIDTHS:
        got, res = run(lib, keys, idx, sig, msg, SEEDS[5], c)
        assert res == 1 and np.array_equal(got, bm.encode(want)), c


@pytest.mark.parametrize("what", ["named key", "S = L", "R", "index", "all of one key"])
def test_rejected_elements_give_zero_and_are_left_out_of_the_point(lib, oracle, what):
    """"all of one key": a key named only by rejected elements has sum zero and yields no digits"""
    keys, idx, sig, msg = (a.copy() for a in honest(oracle, 12, 4, 0xC0A1E5D2))
    if what == "named key":
        keys[2] = bm.undecodable()                                                # elements 2, 6, 10
    elif what == "S = L":
        sig[4, 32:] = np.frombuffer(L.to_bytes(32, "little"), np.uint8)
    elif what == "R":
        sig[4, :32] = bm.undecodable()
    elif what == "index":
        idx[4] = len(keys)
    else:
        sig[[1, 5, 9], 32:] = np.frombuffer(L.to_bytes(32, "little"), np.uint8)   # every element of key 1
    want, ok = im.batch_point(keys, idx, sig, msg, SEEDS[6])
    assert not ok and im.batch_result(keys, idx, sig, msg, SEEDS[6]) == 0 == im.gathered_result(keys, idx, sig, msg, SEEDS[6])
    for c in WIDTHS:
        got, res = run(lib, keys, idx, sig, msg, SEEDS[6], c)
        assert res == 0 and np.array_equal(got, bm.encode(want)), (what, c)
    # ... and what is left satisfies the equation: the point is in the 8-torsion
    assert bm._affine(bm._mul(8, bm._ext(want))) == (0, 1)


def test_the_same_bytes_at_two_indices_are_two_points(lib, oracle):
    keys, idx, sig, msg = honest(oracle, 10, 1, 0xC0A1E5D4)
    keys2 = np.concatenate([keys, keys])
    idx2 = (np.arange(10) % 2).astype(np.uint32)
    want, ok = im.batch_point(keys2, idx2, sig, msg, SEEDS[7])
    got, res = run(lib, keys2, idx2, sig, msg, SEEDS[7], 8)
    assert ok and res == 1 and np.array_equal(got, bm.encode(want))


# ---- the closed form (tests/batch_eq_model.py): exact points where the buckets fill ----------------------------------------
# Honest keys have prime order, so the coalesced point of shifted honest rows is the un-indexed one: [sum z_i d_i mod L]B.
# The host *_batch forms draw their seeds inside the library and cannot be steered: they are out of scope here.

CLOSED_FORM = ((1000, 7), (1000, 8), (3000, 10), (3000, 13))               # (n, c), as tests/test_host_emul_verify_batch.py
KEY_COUNTS = (1, 7, None)                                                   # one hot key (every term merged), seven, one per element


@pytest.fixture(scope="module")
def exact(oracle):
    """K -> 3000 honest signatures over K keys (None: 3000), each exactly valid under the reference's cofactorless equation; element i
    names key i mod K, so the first n elements name the first min(n, K) keys"""
    out = {}
    for j, K in enumerate(KEY_COUNTS):
        keys, idx, sig, msg = honest(oracle, 3000, K or 3000, 0xC0A1E5E0 + 2 * j)
        assert oracle.ed25519_verify(sig, keys[idx], msg, threads=4).all()
        out[K] = keys, idx, sig, msg
    return out


@pytest.mark.parametrize("K", KEY_COUNTS)
@pytest.mark.parametrize("n,c", CLOSED_FORM)
def test_shifted_rows_give_the_closed_form_point(lib, exact, n, c, K):
    """every S moved by an odd 62-bit delta, three rows rejected away from the ends: T = [sum z_i d_i]B over the rows that stay"""
    keys, idx, sig, msg = exact[K]
    keys, idx, sig, msg = keys[:K or n], idx[:n].copy(), sig[:n], msg[:n]
    out = {n // 3: "S = L", n // 2: "index", 2 * n // 3 + 1: "R"}
    rows = [i for i in range(n) if i not in out]
    deltas = bm.odd_deltas(len(rows), 0xC0A1E5E8 + n + c)
    sig = bm.shift_s(sig, rows, deltas)
    for row, what in out.items():
        if what == "S = L":
            sig[row, 32:] = np.frombuffer(L.to_bytes(32, "little"), np.uint8)
        elif what == "index":
            idx[row] = len(keys)
        else:
            sig[row, :32] = bm.undecodable()
    want = bm.shifted_point(bm.shift_sums(SEEDS[4], rows, deltas), n)
    got, res = run(lib, keys, idx, sig, msg, SEEDS[4], c)
    assert res == 0 and np.array_equal(got, bm.encode(want)), (n, c, K)


@pytest.mark.parametrize("K", KEY_COUNTS)
@pytest.mark.parametrize("n,c", CLOSED_FORM)
def test_a_steered_batch_is_accepted(lib, exact, n, c, K):
    """every S moved, the last row's by the delta that makes sum z_i d_i = 0 mod L: no element is valid, T is the neutral element and
    the result 1 -- the defined behaviour of a batch rule under a KNOWN seed (callers pass secret ones); it holds only if every z_i,
    every k_i and every key's merged sum is the right one"""
    keys, idx, sig, msg = exact[K]
    keys, idx, sig, msg = keys[:K or n], idx[:n], sig[:n], msg[:n]
    rows = list(range(n))
    deltas = bm.odd_deltas(n, 0xC0A1E5E9 + n + c)
    deltas[n - 1] = bm.steering_delta(SEEDS[5], bm.shift_sums(SEEDS[5], rows, deltas), n, n - 1)
    steered = bm.shift_s(sig, rows, deltas)
    assert bm.shifted_point(bm.shift_sums(SEEDS[5], rows, deltas), n) == (0, 1)
    pick = [0, 1, n // 2, n - 2, n - 1]
    assert not zc.zip215_rule(steered[pick], keys[idx[pick]], msg[pick]).any()
    got, res = run(lib, keys, idx, steered, msg, SEEDS[5], c)
    assert res == 1 and np.array_equal(got, bm.encode((0, 1))), (n, c, K)
