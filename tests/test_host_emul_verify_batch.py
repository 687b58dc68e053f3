"""CPU tests of the ZIP-215 batch equation (what ed25519_VerifyBatch_zip215_* runs on the device above BATCH_EQ_MIN).  The lane-level
device source, curve25519_amd/csrc/msm25519.cuh, is compiled by g++ against the C model of the gfx950 primitives
(tests/host_emul/verify_batch.cpp, tests/host_emul/build.py's build_lib); a host counting sort stands in for the kernels' atomics.
Expected points and results: the rule in Python big integers (tests/batch_eq_model.py)."""
import ctypes as C
import random

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import batch_eq_model as bm
import zip215_cases as zc
from vectors import L

vp, sz = C.c_void_p, C.c_size_t
WIDTHS = (8, 10, 13)
SEEDS = [bytes([17 * j + 1]) * 32 for j in range(8)]


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_batcheq_digits": [vp, vp, C.c_int, C.c_int], "emul_batcheq_top_range": [C.c_int, C.c_int],
                    "emul_batcheq": [vp, vp, vp, vp, sz, sz, vp, C.c_int]},
                   "verify_batch.cpp", "libc25519_emul_verify_batch.so")
    yield lib
    assert_no_mad_overflow(lib)


def ptr(a):
    return a.ctypes.data_as(vp)


def run(lib, sig, pk, msg, seed, c):
    """(enc(T), result) of the emulated chain"""
    sig, pk, msg = (np.ascontiguousarray(a, np.uint8) for a in (sig, pk, msg))
    point = np.zeros(32, np.uint8)
    sd = np.frombuffer(seed, np.uint8).copy()
    res = lib.emul_batcheq(ptr(point), ptr(sig), ptr(pk), ptr(msg), msg.shape[1], len(sig), ptr(sd), c)
    return point, res


def honest(oracle, n, seed):
    pub, priv = oracle.ed25519_keypair(oracle.random_bytes((n, 32), seed))
    msg = oracle.random_bytes((n, 32), seed + 1)
    return oracle.ed25519_sign(priv, msg), pub, msg


@pytest.fixture(scope="module")
def inputs(oracle):
    """the five all-valid inputs: name -> (sig, pk, msg[n, 32])"""
    h = honest(oracle, 48, 0xBA7C4001)
    gsig, gpk, _ = (a[::7] for a in zc.conformance_grid())
    g = gsig, gpk, oracle.random_bytes((len(gsig), 32), 0xBA7C4003)            # S = 0 on small-order points: valid under any message
    t = zc.torsion()
    one = tuple(np.repeat(a[5:6], 32, axis=0) for a in h)
    cat = tuple(np.concatenate(parts) for parts in zip(h, g, t, one))
    perm = np.random.default_rng(0xBA7C4004).permutation(len(cat[0]))
    out = {"honest": h, "grid": g, "torsion": t, "copies": one, "mixed": tuple(a[perm] for a in cat)}
    assert len(g[0]) == 28 and len(t[0]) == 24 and t[2].shape[1] == 32
    for name, (sig, pk, msg) in out.items():
        if name != "mixed":
            assert zc.zip215_rule(sig, pk, msg).all(), name
    return out


# ---- digits ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", range(7, 14))
def test_digits_recompose_the_scalar_and_stay_within_half_a_window(lib, c):
    """every width BATCH_EQ_WINDOW accepts (MSM_C_MIN .. MSM_C_MAX).  The top digit of a scalar the kernels can meet -- an a_i below L, a
    z_i below 2^128 -- also stays within R, the range its window's sub-buckets are cut for (msm_slot would clamp a larger one)"""
    rnd = random.Random(0xD161 + c)
    scalars = [0, 1, 2**128 - 1, 2**128, L - 1, 2**253 - 1]
    scalars += [sum(((1 << c) - 1) << (c * w) for w in range(0, 253 // c, 2)), sum(((1 << c) - 1) << (c * w) for w in range(1, 253 // c, 2)),
                (1 << (c * (253 // c))) - 1]                                      # all-ones windows: every other one, and a full run
    scalars += [rnd.getrandbits(253) for _ in range(100)] + [rnd.getrandbits(253) % L for _ in range(100)]
    scalars += [L - 1 - j for j in range(1, 4)] + [2**252 + j for j in range(-2, 3)] + [2**128 - 1 - j for j in range(1, 4)]
    digits = np.zeros(40, np.int32)
    for k in scalars:
        forms = (0, 1) if k < 2**128 else (0,)
        for as_z in forms:
            raw = np.frombuffer(k.to_bytes(32, "little"), np.uint8).copy()
            nwin = lib.emul_batcheq_digits(ptr(digits), ptr(raw), c, as_z)
            assert nwin == (-(-130 // c) if as_z else -(-255 // c))
            d = [int(x) for x in digits[:nwin]]
            assert sum(x << (c * w) for w, x in enumerate(d)) == k, (hex(k), as_z)
            assert max(abs(x) for x in d) <= 1 << (c - 1), (hex(k), as_z)
            if as_z or k < L:
                assert 0 <= d[-1] <= lib.emul_batcheq_top_range(c, as_z) <= 1 << (c - 1), (hex(k), as_z)
    digits_z = np.zeros(40, np.int32)
    raw = np.frombuffer((2**128 - 1).to_bytes(32, "little"), np.uint8).copy()
    assert lib.emul_batcheq_digits(ptr(digits_z), ptr(raw), c, 1) < lib.emul_batcheq_digits(ptr(digits), ptr(raw), c, 0)


# ---- the chain against the model ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("name", ["honest", "grid", "torsion", "copies", "mixed"])
def test_point_equals_the_model(lib, inputs, name, c):
    sig, pk, msg = inputs[name]
    want, ok = bm.batch_point(sig, pk, msg, SEEDS[0])
    got, res = run(lib, sig, pk, msg, SEEDS[0], c)
    assert ok and np.array_equal(got, bm.encode(want)), (name, c)
    assert res == 1


@pytest.mark.parametrize("name", ["honest", "grid", "torsion", "copies", "mixed"])
def test_result_equals_the_model_for_three_seeds(lib, inputs, name):
    sig, pk, msg = inputs[name]
    for j, seed in enumerate(SEEDS[1:4]):
        want = bm.batch_result(sig, pk, msg, seed)
        assert want == 1
        assert run(lib, sig, pk, msg, seed, WIDTHS[j])[1] == want, (name, j)
    bad = sig.copy()
    bad[len(bad) // 2, 40] ^= 0x04                                                # one S off: the model and the chain say 0
    for j, seed in enumerate(SEEDS[1:4]):
        assert bm.batch_result(bad, pk, msg, seed) == 0
        assert run(lib, bad, pk, msg, seed, WIDTHS[j])[1] == 0, (name, j)


def test_cancelling_pair_is_rejected_for_eight_seeds(lib, oracle):
    sig, pk, msg = bm.cancelling_pair(oracle)
    assert zc.zip215_rule(sig, pk, msg).tolist() == [0, 0]
    for j, seed in enumerate(SEEDS):
        assert bm.batch_result(sig, pk, msg, seed) == 0
        assert run(lib, sig, pk, msg, seed, WIDTHS[j % 3])[1] == 0, j


def test_torsion_shifted_pair_is_accepted(lib, oracle):
    sig, pk, msg = bm.torsion_pair()
    assert zc.zip215_rule(sig, pk, msg).tolist() == [1, 1]
    assert oracle.ed25519_verify(sig, pk, msg).tolist() == [0, 0]                 # the cofactorless equation rejects both
    for c in WIDTHS:
        assert run(lib, sig, pk, msg, SEEDS[2], c)[1] == 1 == bm.batch_result(sig, pk, msg, SEEDS[2])


@pytest.mark.parametrize("what", ["S = L", "key", "R"])
def test_rejected_elements_give_zero_and_are_left_out_of_the_point(lib, oracle, what):
    sig, pk, msg = (a.copy() for a in honest(oracle, 9, 0xBA7C4010))
    if what == "S = L":
        sig[4, 32:] = np.frombuffer(L.to_bytes(32, "little"), np.uint8)
    elif what == "key":
        pk[4] = bm.undecodable()
    else:
        sig[4, :32] = bm.undecodable()
    want, ok = bm.batch_point(sig, pk, msg, SEEDS[3])
    assert not ok and bm.batch_result(sig, pk, msg, SEEDS[3]) == 0
    for c in WIDTHS:
        got, res = run(lib, sig, pk, msg, SEEDS[3], c)
        assert res == 0 and np.array_equal(got, bm.encode(want)), (what, c)
    # ... and what is left satisfies the equation: the point is in the 8-torsion
    assert bm._affine(bm._mul(8, bm._ext(want))) == (0, 1)


# ---- the closed form (tests/batch_eq_model.py): exact points where the buckets fill ----------------------------------------
# The host *_batch forms draw their seeds inside the library and cannot be steered: they are out of scope here.

CLOSED_FORM = ((1000, 7), (1000, 8), (3000, 10), (3000, 13))               # (n, c): chains in the buckets, the p mod G split, dense chunks


@pytest.fixture(scope="module")
def exact(oracle):
    """3000 honest signatures, each exactly valid under the reference's cofactorless equation"""
    sig, pk, msg = honest(oracle, max(n for n, _ in CLOSED_FORM), 0xBA7C4020)
    assert oracle.ed25519_verify(sig, pk, msg, threads=4).all()
    return sig, pk, msg


@pytest.mark.parametrize("n,c", CLOSED_FORM)
def test_shifted_rows_give_the_closed_form_point(lib, exact, n, c):
    """every S moved by an odd 62-bit delta, three rows rejected away from the ends: T = [sum z_i d_i]B over the rows that stay"""
    sig, pk, msg = (a[:n].copy() for a in exact)
    out = {n // 3: "S = L", n // 2: "key", 2 * n // 3 + 1: "R"}
    rows = [i for i in range(n) if i not in out]
    deltas = bm.odd_deltas(len(rows), 0xBA7C4021 + n + c)
    sig = bm.shift_s(sig, rows, deltas)
    for row, what in out.items():
        if what == "S = L":
            sig[row, 32:] = np.frombuffer(L.to_bytes(32, "little"), np.uint8)
        elif what == "key":
            pk[row] = bm.undecodable()
        else:
            sig[row, :32] = bm.undecodable()
    want = bm.shifted_point(bm.shift_sums(SEEDS[4], rows, deltas), n)
    got, res = run(lib, sig, pk, msg, SEEDS[4], c)
    assert res == 0 and np.array_equal(got, bm.encode(want)), (n, c)


def any_sampled_row_valid(sig, pk, msg):
    """the ZIP-215 rule accepts one of five rows on its own (the ends and the middle)"""
    pick = [0, 1, len(sig) // 2, len(sig) - 2, len(sig) - 1]
    return zc.zip215_rule(sig[pick], pk[pick], msg[pick]).any()


@pytest.mark.parametrize("n,c", CLOSED_FORM)
def test_a_steered_batch_is_accepted_and_one_more_step_is_not(lib, exact, n, c):
    """every S moved, the last row's by the delta that makes sum z_i d_i = 0 mod L: no element is valid, T is the neutral element and
    the result 1 -- the defined behaviour of a batch rule under a KNOWN seed (callers pass secret ones); it holds only if every z_i
    and every k_i is the right one.  With a middle row's S one further, the result is 0."""
    sig, pk, msg = (a[:n] for a in exact)
    rows = list(range(n))
    deltas = bm.odd_deltas(n, 0xBA7C4022 + n + c)
    deltas[n - 1] = bm.steering_delta(SEEDS[5], bm.shift_sums(SEEDS[5], rows, deltas), n, n - 1)
    steered = bm.shift_s(sig, rows, deltas)
    assert bm.shifted_point(bm.shift_sums(SEEDS[5], rows, deltas), n) == (0, 1)
    assert not any_sampled_row_valid(steered, pk, msg)
    got, res = run(lib, steered, pk, msg, SEEDS[5], c)
    assert res == 1 and np.array_equal(got, bm.encode((0, 1))), (n, c)
    if (n, c) == CLOSED_FORM[-1]:                                                 # (one such run is enough on the CPU)
        bumped = bm.shift_s(steered, [n // 2 + 7], [1])
        assert run(lib, bumped, pk, msg, SEEDS[5], c)[1] == 0, (n, c)
