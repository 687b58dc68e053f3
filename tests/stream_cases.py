"""Inputs, call sequences and expected bytes for the device-pointer calls issued on several streams of one thread
(tests/test_gpu_streams.py runs them on the device; tests/test_stream_cases.py checks with the oracle and the models alone what
that module's assertions rest on).  No GPU in here: seeds come from synth.random_bytes, keys and signatures from the oracle.

Every verification row is an oracle signature under an oracle key, rejected -- where it is -- through ONE flipped bit in R, in S
below byte 63 or in the last message byte, so the plain, the strict and the ZIP-215 rule give the same verdict and the oracle's
verdict serves all three forms of a call.

Three kinds of input:
  one_key_sets   two keys K0, K1 with a block of BLOCK oracle-checked rows each, tiled to the size of a call: what the calls that
                 hand the kept comb of ed25519_Verify_Check_*dev from stream to stream verify
  one_peer_sets  two peers on the curve, one on the twist and u = p - 1, with one block of secrets: the same for
                 curve25519_dh_CreateSharedKey_one_peer_dev
  rotation_set   ROT_LARGE rows (the first ROT_SMALL are the small size) for every other *_dev call, the verification rows tiled
                 from ROT_DISTINCT distinct ones so that all three rule sets are modelled on every row
and, for each kept buffer, a model of which calls walk the comb (check_paths, peer_paths): the host knows the size, the device
compares the key with the remembered one."""
import functools
import hashlib

import numpy as np

import key_model
import one_peer_cases as opc
from curve25519_amd import synth
from dispatch_cases import MASK255, THREADS, _flip_m, _flip_r, _flip_s, _le
from vectors import P, ed_decode

# ---- sizes --------------------------------------------------------------------------------------------------------------------
ONE_KEY_WIDE = 1 << 16                   # the default of the tunable: ed25519_Verify_Check_* builds a comb for its key from here on
ONE_PEER_WIDE = 3 << 15                  # ... and curve25519_dh_CreateSharedKey_one_peer_* for a new peer
COOP_MAX = 1024                          # up to here a call runs one element per wave and asks nothing of the kept buffer
BLOCK = 1 << 15                          # rows the oracle computes per key / per peer
A_ROWS = 1 << 17                         # call A: long enough to be walking its comb while the next call is enqueued
PEER_A_ROWS = 1 << 19                    # ... the peer's comb is walked ten times as fast as the key's: 2^17 secrets take 0.1 ms
SMALL = 4096                             # a call below the build size: the device compares its key with the remembered one
MSG_LEN = 32
ROT_SMALL, ROT_LARGE = 700, 9000         # the rotation's sizes: four lanes per element, and one
ROT_DISTINCT = 256
ROT_KEYS = 8
ROT_MSG_LEN = 48
GARBAGE_EVERY, GARBAGE_FIRST = 1000, 5   # garbage keys in the plain and the ZIP-215 per-element verification: the slow list


def tile(a, n):
    """n rows: a's rows again and again"""
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


def reject_rows(sig, msg):
    """one flipped bit in R at rows 7k, in S (bytes 32..62) at 7k + 2, in the last message byte at 7k + 4"""
    for i in range(0, len(sig), 7):
        _flip_r(sig, i)
    for i in range(2, len(sig), 7):
        _flip_s(sig, i)
    for i in range(4, len(sig), 7):
        _flip_m(msg, i)


# ---- a: one key per call ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_key_sets(oracle):
    """[(pub uint8[1, 32], sig uint8[BLOCK, 64], msg uint8[BLOCK, MSG_LEN], verdict int32[BLOCK])] for K0 and K1"""
    pub, priv = oracle.ed25519_keypair(synth.random_bytes((2, 32), 0x57A00001), threads=THREADS)
    out = []
    for k in range(2):
        msg = synth.random_bytes((BLOCK, MSG_LEN), 0x57A10000 + k)
        sig = oracle.ed25519_sign(np.repeat(priv[k:k + 1], BLOCK, axis=0), msg, threads=THREADS)
        reject_rows(sig, msg)
        ok = oracle.ed25519_verify(sig, np.repeat(pub[k:k + 1], BLOCK, axis=0), msg, threads=THREADS)
        for a in (sig, msg, ok):
            a.setflags(write=False)
        out.append((pub[k:k + 1].copy(), sig, msg, ok))
    return out


# name -> (key, rows).  A builds K0's comb and walks it; B rebuilds the buffer for K1; C asks for K0 below the build size; D for K1
VERIFY_CALLS = {"A": (0, A_ROWS), "B": (1, ONE_KEY_WIDE), "C": (0, SMALL), "D": (1, SMALL)}
# scenario -> [(call, stream)] in issue order.  one_stream is the control: stream order alone keeps it right
VERIFY_ORDERS = {
    "handover": (("A", 0), ("B", 1), ("C", 2), ("D", 0)),
    "swapped": (("A", 1), ("B", 0), ("C", 2), ("D", 1)),
    "b_first": (("B", 1), ("A", 0), ("C", 2), ("D", 0)),
    "one_stream": (("A", 0), ("B", 0), ("C", 0), ("D", 0)),
}


def check_paths(calls, wide_from=ONE_KEY_WIDE):
    """what c25519_amd_verify_check_last_wide says after each (key, rows) of a thread that starts with nothing kept, every key being
    Verify_Init's context of a key on the curve: a call of wide_from rows builds the comb for its key (or finds it), a smaller one
    above the per-wave range walks the kept comb if the remembered context is its own"""
    remembered, out = None, []
    for key, rows in calls:
        if rows >= wide_from:
            remembered = key
            out.append(1)
        else:
            out.append(int(rows > COOP_MAX and remembered is not None and key == remembered))
    return out


# ---- b: one peer per call -----------------------------------------------------------------------------------------------------
PEER_TWIST = opc.to_bytes(opc.TWIST[0])
PEER_MINUS_ONE = opc.to_bytes(P - 1)


@functools.lru_cache(maxsize=None)
def one_peer_sets(oracle):
    """(sk uint8[BLOCK, 32], {name: (pk uint8[1, 32], shared uint8[BLOCK, 32], clamped sk)}) for the peers p0, p1 (public keys the
    oracle computes from seeded secrets), twist and minus_one"""
    sk = synth.random_bytes((BLOCK, 32), 0x57A20000)
    pub, _ = oracle.x25519_public(synth.random_bytes((2, 32), 0x57A20001))
    peers = {"p0": pub[0].tobytes(), "p1": pub[1].tobytes(), "twist": PEER_TWIST, "minus_one": PEER_MINUS_ONE}
    out = {}
    for name, pk in peers.items():
        row = np.frombuffer(pk, np.uint8).reshape(1, 32).copy()
        shared, clamped = oracle.x25519_shared(np.repeat(row, BLOCK, axis=0), sk, threads=THREADS)
        shared.setflags(write=False)
        clamped.setflags(write=False)
        out[name] = (row, shared, clamped)
    sk.setflags(write=False)
    return sk, out


# T and M are refused by the device: the ladder decides them, and the last refused key is written into the kept buffer.
# A call whose verdict is "the ladder" (T, M, C) writes 0 into the `flags` words that the kept buffer holds for all calls, and every
# comb kernel that finds 0 there leaves its call to the ladder, which is always right.  Run early on a stream of its own, such a
# call would hide a missing wait between A and B -- so in the first three orders everything but A and B is stream-ordered behind
# one of the two, and while A walks its comb nothing but B's rebuild can touch the buffer; third_stream keeps a's shape.
PEER_CALLS = {"A": ("p0", PEER_A_ROWS), "B": ("p1", ONE_PEER_WIDE), "T": ("twist", ONE_PEER_WIDE), "M": ("minus_one", ONE_PEER_WIDE),
              "C": ("p0", SMALL), "D": ("p1", SMALL)}
PEER_ORDERS = {
    "handover": (("A", 0), ("B", 1), ("T", 0), ("M", 1), ("C", 0), ("D", 1)),
    "swapped": (("A", 1), ("B", 0), ("T", 1), ("M", 0), ("C", 1), ("D", 0)),
    "b_first": (("B", 1), ("A", 0), ("T", 1), ("M", 0), ("C", 1), ("D", 0)),
    "third_stream": (("A", 0), ("B", 1), ("T", 2), ("M", 0), ("C", 2), ("D", 0)),
    "one_stream": tuple((c, 0) for c in "ABTMCD"),
}
# c: both kept buffers at once, a's and b's calls in turn over three streams
BOTH_ORDER = tuple((kind, call, i % 3) for i, (kind, call) in enumerate(
    [("verify", "A"), ("peer", "A"), ("verify", "B"), ("peer", "B"), ("peer", "T"), ("verify", "C"), ("peer", "M"), ("verify", "D"),
     ("peer", "C"), ("peer", "D")]))


def peer_paths(calls, wide_from=ONE_PEER_WIDE):
    """what c25519_amd_x25519_one_peer_last_wide says after each (peer name, rows), as check_paths: an ineligible peer (off the
    curve, or u = -1) builds nothing and leaves the remembered peer where it was"""
    remembered, kept, out = None, False, []
    for name, rows in calls:
        if rows >= wide_from:
            kept = True
            if name != remembered and peer_eligible(name):
                remembered = name
            out.append(int(name == remembered))
        else:
            out.append(int(rows > COOP_MAX and kept and name == remembered))
    return out


def peer_eligible(name):
    return name in ("p0", "p1")


# ---- d: every other call ------------------------------------------------------------------------------------------------------
def undecodable(key_row):
    v = int.from_bytes(bytes(key_row), "little")
    return ed_decode((v & MASK255) % P, v >> 255) is None


@functools.lru_cache(maxsize=None)
def rotation_set(oracle):
    """a dict of uint8 / int32 arrays of ROT_LARGE rows (a call of ROT_SMALL rows takes the first ROT_SMALL):
    keys of ROT_KEYS signers and peers, idx which of them a row uses, clean messages and their oracle signatures, the verification
    rows (tiled from ROT_DISTINCT distinct ones) with the oracle's verdicts, the same with garbage keys, and the expected bytes of
    every call of the rotation"""
    n = ROT_LARGE
    d = {}
    d["esk"] = synth.random_bytes((ROT_KEYS, 32), 0x57A30001)
    d["pub"], d["priv"] = oracle.ed25519_keypair(d["esk"], threads=THREADS)
    d["idx"] = (synth.random_bytes((n, 1), 0x57A30002) % ROT_KEYS).astype(np.uint32)
    idx = d["idx"].reshape(n)
    d["priv_rows"] = np.ascontiguousarray(d["priv"][idx])
    # signing: clean messages
    d["msg"] = synth.random_bytes((n, ROT_MSG_LEN), 0x57A30003)
    d["sig"] = oracle.ed25519_sign(d["priv_rows"], d["msg"], threads=THREADS)
    # verification: ROT_DISTINCT distinct rows, tiled.  Row j of the tile keeps the key idx[j % ROT_DISTINCT]
    vidx = idx[:ROT_DISTINCT]
    vmsg = d["msg"][:ROT_DISTINCT].copy()
    vsig = d["sig"][:ROT_DISTINCT].copy()
    reject_rows(vsig, vmsg)
    vpk = np.ascontiguousarray(d["pub"][vidx])
    d["v_distinct"] = (vsig, vpk, vmsg)
    d["v_idx"] = tile(vidx.reshape(-1, 1), n)
    d["v_sig"], d["v_pk"], d["v_msg"] = tile(vsig, n), tile(vpk, n), tile(vmsg, n)
    d["v_ok"] = tile(oracle.ed25519_verify(vsig, vpk, vmsg, threads=THREADS), n)
    d["g_pk"] = d["v_pk"].copy()
    d["g_rows"] = np.arange(GARBAGE_FIRST, n, GARBAGE_EVERY)
    d["g_pk"][d["g_rows"]] = synth.random_bytes((len(d["g_rows"]), 32), 0x57A30004)
    d["g_ok"] = oracle.ed25519_verify(d["v_sig"], d["g_pk"], d["v_msg"], threads=THREADS)
    # the batch equation: the accepted rows alone (result 1), and all rows (result 0)
    d["valid_rows"] = np.flatnonzero(d["v_ok"] == 1)
    # X25519: ROT_KEYS peers (public keys of seeded secrets), one secret per row
    d["xpk"], _ = oracle.x25519_public(synth.random_bytes((ROT_KEYS, 32), 0x57A30005))
    d["xsk"] = synth.random_bytes((n, 32), 0x57A30006)
    d["shared"], d["xsk_clamped"] = oracle.x25519_shared(np.ascontiguousarray(d["xpk"][idx]), d["xsk"], threads=THREADS)
    # key pairs and public keys of one secret per row
    d["kp_pub"], d["kp_priv"] = oracle.ed25519_keypair(d["xsk"], threads=THREADS)
    d["x_pub"], _ = oracle.x25519_public(d["xsk"], fast=False, threads=THREADS)
    d["x_pub_fast"], _ = oracle.x25519_public(d["xsk"], fast=True, threads=THREADS)
    # classification and conversion: the model's case set, tiled
    keys, _ = key_model.case_set()
    flags, xpk, ok = key_model.expected(keys)
    d["c_keys"], d["c_flags"], d["c_xpk"], d["c_ok"] = tile(keys, n), tile(flags, n), tile(xpk, n), tile(ok, n)
    seeds = {k: key_model.private_to_x25519(bytes(d["priv"][k])) for k in range(ROT_KEYS)}
    d["c_xsk"] = np.stack([np.frombuffer(seeds[int(k)], np.uint8) for k in idx])
    assert all(seeds[k] == _clamped_hash(bytes(d["esk"][k])) for k in range(ROT_KEYS))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _clamped_hash(seed):
    h = bytearray(hashlib.sha512(seed).digest()[:32])
    h[0] &= 248
    h[31] = (h[31] & 127) | 64
    return bytes(h)


def ragged_offsets(n, width):
    """every message `width` bytes long, as the offsets of a ragged call: uint64[n + 1]"""
    return (np.arange(n + 1, dtype=np.uint64) * np.uint64(width)).reshape(-1, 1)


def slow_rows(d, m):
    """how many of the first m rows of the garbage-key set the plain call sends to its slow list: the keys that do not decode"""
    return sum(1 for r in d["g_rows"] if r < m and undecodable(d["g_pk"][r]))


assert _le(P - 1).tobytes() == PEER_MINUS_ONE
