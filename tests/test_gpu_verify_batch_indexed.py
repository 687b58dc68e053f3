"""GPU suite (MI355X): ZIP-215 batch verification with coalesced keys -- ed25519_VerifyBatch_zip215_indexed_batch / _dev /
_ragged_batch / _ragged_dev and the hook c25519_amd_verify_batch_indexed_point_dev.  Expected points: tests/batch_eq_indexed_model.py;
expected results: the model's for the small shapes, and for every shape what ed25519_VerifyBatch_zip215_dev gives on the gathered keys
with the same seed.  At scale the point is pinned by the closed form of tests/batch_eq_model.py (rows whose S is moved by a known
delta), with the rows of the special keys through the coalesced model on that subset.  The host *_batch forms draw their seeds inside
the library and cannot be steered: the closed form stays with the *_dev form and the hook.  Every case is a well-formed call."""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

import batch_eq_indexed_model as im
import batch_eq_model as bm
import zip215_cases as zc
from curve25519_amd import _lib

pytestmark = pytest.mark.gpu

# where the combining inside a wave and a 256-lane workgroup, a single hot key and all-distinct keys can each go wrong
HOOK_SHAPES = ((1, 1), (2, 1), (64, 1), (65, 2), (257, 3), (600, 1), (600, 7), (600, 600))
EQUAL_SHAPES = ((4099, 5), (4099, 300), (32769, 1), (65537, 4096))
PATTERNS = ("mod", "runs", "random")
# the closed form: a hot key that sums 65537 terms per 32-bit word, all-distinct keys, and 1024 terms per key under every pattern
CLOSED_SHAPES = tuple((n, K, "random") for n, K in EQUAL_SHAPES) + ((65537, 1, "mod"), (65537, 65537, "random")) \
    + tuple(((1 << 18) + 5, 256, pattern) for pattern in PATTERNS)
WIDTHS = (8, 10, 13, None)
SEEDS = [bytes([31 * j + 7]) * 32 for j in range(3)]
MIN_DEFAULT = 1 << 18                   # the default BATCH_EQ_INDEXED_MIN (test_default_tunables pins it)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@contextlib.contextmanager
def tunables(**kv):
    with contextlib.ExitStack() as st:
        for k, v in kv.items():
            st.enter_context(_lib.tunable(k, v))
        yield


def dev(*arrays):
    import torch
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32).reshape(-1, 1)
        out.append(torch.from_numpy(a).cuda())
    return tuple(out)


def result_dev(api, keys, idx, sig, msg, seed):
    """ed25519_VerifyBatch_zip215_indexed_dev on device tensors -> int"""
    import torch
    res = torch.full((1, 1), -7, dtype=torch.int32, device=sig.device)
    api.ed25519_VerifyBatch_zip215_indexed_dev(res, keys, idx, sig, msg, seed)
    return int(res.cpu()[0, 0])


def plain_result_dev(api, keys, idx, sig, msg, seed):
    """the existing call on the gathered keys, forced to run its equation"""
    import torch
    res = torch.full((1, 1), -7, dtype=torch.int32, device=sig.device)
    pk = keys[idx.reshape(-1).long()].contiguous()
    with tunables(BATCH_EQ_MIN=1):
        api.ed25519_VerifyBatch_zip215_dev(res, sig, pk, msg, seed)
    return int(res.cpu()[0, 0])


def point_dev(api, keys, idx, sig, msg, seed):
    import torch
    out = torch.zeros((1, 32), dtype=torch.uint8, device=sig.device)
    api.verify_batch_indexed_point_dev(out, keys, idx, sig, msg, seed)
    return out.cpu().numpy()[0]


@pytest.fixture(scope="module")
def special():
    """the rows mixed into the honest ones: per mixed-order key of zc.torsion() its (sig, msg) rows, and two small-order keys of the
    conformance grid with grid signatures (S = 0 and a small-order R: valid under any small-order key and any message)"""
    tsig, tpk, tmsg = zc.torsion()
    tkeys, tidx = im.distinct_keys(tpk)
    assert len(tkeys) == 3
    rows = [(tkeys[j], tsig[tidx == j], tmsg[tidx == j]) for j in range(3)]
    gsig, gpk, _ = zc.conformance_grid()
    gkeys, _ = im.distinct_keys(gpk)
    gmsg = np.random.default_rng(0x1DE0).integers(0, 256, (len(gsig), 32), dtype=np.uint8)
    for j in (3, 9):
        pick = slice(j, None, 23)
        assert zc.zip215_rule(gsig[pick], np.repeat(gkeys[j][None], len(gsig[pick]), axis=0), gmsg[pick]).all()
        rows.append((gkeys[j], gsig[pick], gmsg[pick]))
    return rows


def key_plan(n, K):
    """key position -> which special key sits there"""
    if (n, K) == (64, 1):
        return {0: 0}                                                             # one hot key of mixed order
    if K in (2, 3):
        return {j: j - 1 for j in range(1, K)}
    if K >= 4:
        return {1: 0, 2: 1, 3: 2, **({5: 3, 6: 4} if K >= 7 else {})}
    return {}


def make(api, special, n, K, pattern, seed):
    """a valid batch: (keys[K, 32], idx uint32[n], sig, msg[n, 32], priv[K, 64])"""
    rng = np.random.default_rng(seed)
    keys, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (K, 32), dtype=np.uint8))
    if pattern == "mod":
        idx = np.arange(n) % K
    elif pattern == "runs":
        idx = np.arange(n) * K // n
    else:
        idx = rng.integers(0, K, n)
    idx = idx.astype(np.uint32)
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sig = api.ed25519_SignMessage(priv[idx], msg)
    for pos, which in key_plan(n, K).items():
        key, ssig, smsg = special[which]
        keys[pos] = key
        at = np.flatnonzero(idx == pos)
        take = np.arange(len(at)) % len(ssig)
        sig[at], msg[at] = ssig[take], smsg[take]
    return keys, idx, sig, msg, priv


@pytest.fixture(scope="module")
def small(api, special):
    """the batch of the rejection, threshold and argument tests: 12 elements over 4 keys (three of them of mixed order)"""
    return make(api, special, 12, 4, "mod", 0x1DE1)


# ---- the hook's point against the model -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K", HOOK_SHAPES)
def test_hook_point_equals_the_model(api, special, n, K):
    for p, pattern in enumerate(PATTERNS if K > 1 else PATTERNS[:1]):
        keys, idx, sig, msg, _ = make(api, special, n, K, pattern, 0x1DE2 + 8 * n + p)
        want, ok = im.batch_point(keys, idx, sig, msg, SEEDS[p])
        assert ok and bm._affine(bm._mul(8, bm._ext(want))) == (0, 1)
        d = dev(keys, idx, sig, msg)
        for c in WIDTHS:
            with tunables(**({} if c is None else {"BATCH_EQ_WINDOW": c})):
                got = point_dev(api, *d, SEEDS[p])
            assert np.array_equal(got, bm.encode(want)), (n, K, pattern, c)
        with tunables(BATCH_EQ_INDEXED_MIN=1):
            assert result_dev(api, *d, SEEDS[p]) == 1
            assert api.verify_batch_last_equation() == 1


def test_hook_point_differs_from_the_plain_one_on_a_mixed_order_key(api, special):
    """the documented torsion remark on the device: one hot key of mixed order, 64 elements -- both results are 1"""
    import torch
    keys, idx, sig, msg, _ = make(api, special, 64, 1, "mod", 0x1DE3)
    d = dev(keys, idx, sig, msg)
    plain = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
    api.verify_batch_point_dev(plain, d[2], d[0][d[1].reshape(-1).long()].contiguous(), d[3], SEEDS[0])
    want_plain, _ = bm.batch_point(sig, keys[idx], msg, SEEDS[0])
    want, _ = im.batch_point(keys, idx, sig, msg, SEEDS[0])
    assert want != want_plain
    assert np.array_equal(plain.cpu().numpy()[0], bm.encode(want_plain))
    assert np.array_equal(point_dev(api, *d, SEEDS[0]), bm.encode(want))
    with tunables(BATCH_EQ_INDEXED_MIN=1):
        assert result_dev(api, *d, SEEDS[0]) == 1 == plain_result_dev(api, *d, SEEDS[0])


# ---- the result equals the existing call's --------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K", EQUAL_SHAPES)
def test_result_equals_the_plain_call_on_the_gathered_keys(api, special, n, K):
    keys, idx, sig, msg, priv = make(api, special, n, K, "random", 0x1DE4 + n + K)
    rng = np.random.default_rng(0x1DE5 + n)
    dk, di, ds, dm = dev(keys, idx, sig, msg)
    with tunables(BATCH_EQ_INDEXED_MIN=1):
        for seed in SEEDS:
            assert result_dev(api, dk, di, ds, dm, seed) == 1 == plain_result_dev(api, dk, di, ds, dm, seed), (n, K)
            assert api.verify_batch_last_equation() == 1
        for row in sorted({0, n - 1, int(rng.integers(0, n))}):
            bad = ds.clone()
            bad[row, 33] ^= 1                                                     # S off by 2^8: no rule accepts the element any more
            assert result_dev(api, dk, di, bad, dm, SEEDS[0]) == 0 == plain_result_dev(api, dk, di, bad, dm, SEEDS[0]), (n, K, row)
        # the one-key cancelling pair: two honest signatures under key 0 with S + 5 and S - 5
        rows = [n // 41, n - 1 - n // 37]
        idx2, sig2, msg2 = idx.copy(), sig.copy(), msg.copy()
        idx2[rows] = 0
        msg2[rows] = rng.integers(0, 256, (2, 32), dtype=np.uint8)
        sig2[rows] = api.ed25519_SignMessage(priv[[0, 0]], msg2[rows])
        for r, delta in zip(rows, (5, -5)):
            S = int.from_bytes(sig2[r, 32:].tobytes(), "little") + delta
            assert 0 <= S < bm.L
            sig2[r, 32:] = np.frombuffer(S.to_bytes(32, "little"), np.uint8)
        assert zc.zip215_rule(sig2[rows], keys[idx2[rows]], msg2[rows]).tolist() == [0, 0]
        d2 = dev(keys, idx2, sig2, msg2)
        for seed in SEEDS:
            assert result_dev(api, *d2, seed) == 0 == plain_result_dev(api, *d2, seed), (n, K)


# ---- the closed form: exact points and steered accepts at scale -------------------------------------------------------------

def s_bytes(sig_row):
    import torch
    return torch.from_numpy(np.ascontiguousarray(sig_row[32:])).cuda()


@pytest.mark.parametrize("n,K,pattern", CLOSED_SHAPES)
def test_shifted_rows_give_the_closed_form_point_and_a_steered_batch_is_accepted(api, oracle, special, n, K, pattern):
    """Honest keys have prime order, so with every honest row's S moved by a known delta the coalesced point is the un-indexed one,
    [sum z_i d_i mod L]B, plus the share of the rows under the special keys (no other row names those): the hook's bytes equal it at
    every width.  Then the last row's delta is chosen so that the sum is 0 mod L: the result is 1 although no honest row is valid --
    the defined behaviour of a batch rule under a KNOWN seed (callers pass secret ones), nothing to be fixed -- and from there one more
    step in the S of any single probed row gives 0.  All of it holds only if every z_i, every k_i and every key's merged sum is exact."""
    import torch
    seed = SEEDS[(n + K) % 3]
    keys, idx, sig, msg, _ = make(api, special, n, K, pattern, 0x1DEC + n + K)
    is_special = np.isin(idx, list(key_plan(n, K)))
    sp, rows = np.flatnonzero(is_special), np.flatnonzero(~is_special).tolist()
    assert oracle.ed25519_verify(sig[rows], keys[idx[rows]], msg[rows], threads=16).all()      # exactly valid, cofactorless
    share = bm._ext(im.batch_point(keys, idx[sp], sig[sp], msg[sp], seed, index=sp)[0]) if len(sp) else bm.NEUTRAL
    assert bm._affine(bm._mul(8, share)) == (0, 1)
    deltas = bm.odd_deltas(len(rows), 0x1DED + n + K)
    host = bm.shift_s(sig, rows, deltas)
    sums = bm.shift_sums(seed, rows, deltas)
    want = bm.encode(bm.shifted_point(sums, n, share))
    dk, di, ds, dm = dev(keys, idx, host, msg)
    for c in WIDTHS:
        with tunables(**({} if c is None else {"BATCH_EQ_WINDOW": c})):
            assert np.array_equal(point_dev(api, dk, di, ds, dm, seed), want), (n, K, pattern, c)
    last = n - 1
    steered = s_bytes(bm.shift_s(sig[last:], [0], [bm.steering_delta(seed, sums, n, last)])[0])
    ds[last, 32:] = steered
    for c in WIDTHS:
        with tunables(BATCH_EQ_INDEXED_MIN=1, **({} if c is None else {"BATCH_EQ_WINDOW": c})):
            assert result_dev(api, dk, di, ds, dm, seed) == 1, (n, K, pattern, c)
            assert api.verify_batch_last_equation() == 1
    assert np.array_equal(point_dev(api, dk, di, ds, dm, seed), bm.encode(bm._affine(share)))
    # every probed row counts: the default width's runs of the digit passes (pts of keyeq_equation) over K keys, then n R's
    more = [int(r) + d for r in sp[:8] for d in (-1, 1)]
    for is_r, q in bm.run_boundary_rows(K, K + n, max(256, 1 << (10 if n < 1 << 16 else 13))):
        more += [q] if is_r else np.flatnonzero(idx == q)[:1].tolist()
    probe = bm.probe_rows(n, more, seed=0x1DEE + n + K)
    assert len(probe) >= 64
    now = host[probe].copy()
    now[probe.index(last), 32:] = steered.cpu().numpy()
    bumped = dev(bm.shift_s(now, range(len(probe)), [1] * len(probe))[:, 32:])[0]
    res = torch.full((4 * len(probe), 1), -7, dtype=torch.int32, device="cuda")    # a result word is 16-byte aligned
    with tunables(BATCH_EQ_INDEXED_MIN=1):
        for j, row in enumerate(probe):
            keep = ds[row, 32:].clone()
            ds[row, 32:] = bumped[j]
            api.ed25519_VerifyBatch_zip215_indexed_dev(res[4 * j:4 * j + 1], dk, di, ds, dm, seed)
            ds[row, 32:] = keep
    wrong = [probe[j] for j in np.flatnonzero(res.cpu().numpy()[::4, 0] != 0)]
    assert not wrong, (n, K, pattern, wrong)


# ---- rejections -----------------------------------------------------------------------------------------------------------

def test_rejected_elements_give_zero_and_the_hook_leaves_them_out(api, small):
    keys, idx, sig, msg, _ = (a.copy() for a in small)
    keys = np.concatenate([keys, bm.undecodable()[None]])                         # key 4: nobody names it yet
    with tunables(BATCH_EQ_INDEXED_MIN=1):
        d = dev(keys, idx, sig, msg)
        assert result_dev(api, *d, SEEDS[1]) == 1                                 # an unnamed undecodable key is not part of the batch
        want, ok = im.batch_point(keys, idx, sig, msg, SEEDS[1])
        assert ok and np.array_equal(point_dev(api, *d, SEEDS[1]), bm.encode(want))

        def spoil(which):
            k, i, s = keys.copy(), idx.copy(), sig.copy()
            if "S = L" in which:
                s[2, 32:] = np.frombuffer(bm.L.to_bytes(32, "little"), np.uint8)
            if "R" in which:
                s[7, :32] = bm.undecodable()
            if "named key" in which:
                i[[4, 9]] = 4
            if "index" in which:
                i[11] = len(k)                                                    # a _dev index = n_key
            return k, i, s, msg

        for which in (("S = L",), ("R",), ("named key",), ("index",), ("S = L", "R", "named key", "index")):
            case = spoil(which)
            want, ok = im.batch_point(*case, SEEDS[1])
            assert not ok and im.gathered_result(*case, SEEDS[1]) == 0
            d = dev(*case)
            assert result_dev(api, *d, SEEDS[1]) == 0, which
            assert np.array_equal(point_dev(api, *d, SEEDS[1]), bm.encode(want)), which
        # a key named only by rejected elements: its sum is zero and it yields no digits
        s3 = sig.copy()
        s3[idx == 3, 32:] = np.frombuffer(bm.L.to_bytes(32, "little"), np.uint8)
        want, ok = im.batch_point(keys, idx, s3, msg, SEEDS[2])
        assert not ok
        d = dev(keys, idx, s3, msg)
        assert result_dev(api, *d, SEEDS[2]) == 0
        assert np.array_equal(point_dev(api, *d, SEEDS[2]), bm.encode(want))


# ---- below BATCH_EQ_INDEXED_MIN -------------------------------------------------------------------------------------------

def test_below_the_threshold_the_per_element_path_gives_the_same_results(api, special):
    for n, K in ((1, 1), (63, 4), (1025, 9)):
        keys, idx, sig, msg, _ = make(api, special, n, K, "random", 0x1DE6 + n)
        dk, di, ds, dm = dev(keys, idx, sig, msg)
        bad = ds.clone()
        bad[n // 2, 33] ^= 1
        out = di.clone()
        out[n - 1, 0] = K                                                         # an index out of range still gives 0
        with tunables(BATCH_EQ_INDEXED_MIN=n + 1):
            assert result_dev(api, dk, di, ds, dm, SEEDS[0]) == 1
            assert api.verify_batch_last_equation() == 0
            assert result_dev(api, dk, di, bad, dm, SEEDS[0]) == 0
            assert result_dev(api, dk, out, ds, dm, SEEDS[0]) == 0
        with tunables(BATCH_EQ_INDEXED_MIN=n):
            assert result_dev(api, dk, di, ds, dm, SEEDS[0]) == 1
            assert api.verify_batch_last_equation() == 1
            assert result_dev(api, dk, out, ds, dm, SEEDS[0]) == 0
        with tunables(BATCH_EQ_INDEXED_MIN=0):                                    # never
            assert result_dev(api, dk, di, bad, dm, SEEDS[0]) == 0
            assert api.verify_batch_last_equation() == 0


def test_default_tunables(api, special):
    """the smallest n that runs the equation with nothing set, over 64 keys"""
    assert _lib.load().c25519_amd_tunable_get(b"BATCH_EQ_INDEXED_MIN") == -1
    keys, idx, sig, msg, _ = make(api, special, MIN_DEFAULT, 64, "random", 0x1DE7)
    dk, di, ds, dm = dev(keys, idx, sig, msg)
    assert result_dev(api, dk, di, ds, dm, SEEDS[2]) == 1
    assert api.verify_batch_last_equation() == 1
    assert result_dev(api, dk, di[:MIN_DEFAULT - 1], ds[:MIN_DEFAULT - 1], dm[:MIN_DEFAULT - 1], SEEDS[2]) == 1
    assert api.verify_batch_last_equation() == 0
    ds[MIN_DEFAULT // 3, 5] ^= 0x20
    assert result_dev(api, dk, di, ds, dm, SEEDS[2]) == 0


# ---- the host forms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K", [(5, 3), (4096, 64), ((1 << 17) + 5, 1000)])
def test_host_form_verdicts_and_null_arguments(api, special, n, K):
    """(2^17 + 5: the call is cut into pieces, one equation each, the element index counting through the call)"""
    keys, idx, sig, msg, _ = make(api, special, n, K, "random", 0x1DE8 + n)
    f = api.ed25519_VerifyBatch_zip215_indexed
    with tunables(BATCH_EQ_INDEXED_MIN=1):
        ok, verdict = f(keys, idx, sig, msg, seed=SEEDS[0], verdicts=True)
        assert ok == 1 and verdict.dtype == np.int32 and (verdict == 1).all()
        assert api.verify_batch_last_equation() == 1
        assert f(keys, idx, sig, msg, seed=SEEDS[1]) == 1                         # a null verdict
        assert f(keys, idx, sig, msg) == 1                                        # a null seed, twice
        assert f(keys, idx, sig, msg) == 1
        bad = sig.copy()
        bad[[0, n // 2, n - 1], 33] ^= 1
        bad[n // 3, 2] ^= 0x40
        ok, verdict = f(keys, idx, bad, msg, seed=SEEDS[0], verdicts=True)
        assert ok == 0 and np.array_equal(verdict, api.ed25519_VerifySignature_zip215(bad, keys[idx], msg)) and (verdict == 0).sum() == 4
        assert f(keys, idx, bad, msg) == 0
        only_last = sig.copy()
        only_last[n - 1, 33] ^= 1                                                 # in the last piece of a call that is cut
        assert f(keys, idx, only_last, msg) == 0
        # an index out of range refuses the call before any work, outputs untouched
        lib = _lib.load()
        out_of_range = idx.copy()
        out_of_range[n - 1] = K
        ok_word, v = C.c_int(-5), np.full(n, -5, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        assert lib.ed25519_VerifyBatch_zip215_indexed_batch(C.byref(ok_word), p(v), p(keys), K, p(out_of_range), p(sig), p(msg), 32, n,
                                                            None) != 0
        assert ok_word.value == -5 and (v == -5).all() and lib.c25519_amd_last_error() != b""
        with pytest.raises(_lib.EngineError):
            f(keys, out_of_range, sig, msg)


def test_ragged_forms_equal_the_fixed_length_forms(api, special):
    import torch
    n, K = 1500, 11
    keys, idx, sig, msg, priv = make(api, special, n, K, "random", 0x1DE9)
    messages = [m.tobytes() for m in msg]
    bad = sig.copy()
    bad[700, 33] ^= 1
    flat, offsets = api._ragged(messages)
    f, g = api.ed25519_VerifyBatch_zip215_indexed_ragged, api.ed25519_VerifyBatch_zip215_indexed
    with tunables(BATCH_EQ_INDEXED_MIN=1):
        assert f(keys, idx, sig, messages, seed=SEEDS[0]) == 1 == g(keys, idx, sig, msg, seed=SEEDS[0])
        ok, verdict = f(keys, idx, bad, messages, verdicts=True)
        assert ok == 0 and np.array_equal(verdict, api.ed25519_VerifySignature_zip215(bad, keys[idx], msg))
        d_flat = torch.from_numpy(flat.reshape(-1, 1).copy()).cuda()
        d_off = torch.from_numpy(offsets.astype(np.int64).reshape(-1, 1)).cuda()
        for s, want in ((sig, 1), (bad, 0)):
            res = torch.full((1, 1), -7, dtype=torch.int32, device="cuda")
            dk, di, dsig = dev(keys, idx, s)
            api.ed25519_VerifyBatch_zip215_indexed_ragged_dev(res, dk, di, dsig, d_flat, d_off, SEEDS[1])
            assert int(res.cpu()[0, 0]) == want
        out_of_range = idx.copy()
        out_of_range[3] = K
        with pytest.raises(_lib.EngineError):
            f(keys, out_of_range, sig, messages)
    # messages of different lengths: the hash sees each one's own bytes
    rng = np.random.default_rng(0x1DEA)
    ragged = [rng.integers(0, 256, i + 1, dtype=np.uint8).tobytes() for i in range(40)]
    idx40 = (np.arange(40) % 4).astype(np.uint32)
    hkeys, hpriv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (4, 32), dtype=np.uint8))
    rsig = api.ed25519_SignMessage_ragged(hpriv[idx40], ragged)
    with tunables(BATCH_EQ_INDEXED_MIN=1):
        assert f(hkeys, idx40, rsig, ragged) == 1
        ragged[20] = ragged[20] + b"x"
        assert f(hkeys, idx40, rsig, ragged) == 0


def test_empty_calls_and_argument_errors(api, small):
    import torch
    lib = _lib.load()
    keys, idx, sig, msg, _ = small
    dk, di, ds, dm = dev(keys, idx, sig, msg)
    e = lambda w, t=np.uint8: np.zeros((0, w), t)  # noqa: E731
    assert api.ed25519_VerifyBatch_zip215_indexed(keys, np.zeros(0, np.uint32), e(64), e(0)) == 1
    assert api.ed25519_VerifyBatch_zip215_indexed(e(32), np.zeros(0, np.uint32), e(64), e(0)) == 1     # n == 0 and no keys
    res = torch.full((4, 1), -7, dtype=torch.int32, device="cuda")
    seed = C.create_string_buffer(SEEDS[0], 32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = (p(res), p(dk), 4, p(di), p(ds), p(dm), 32, 12, seed, st)
    assert lib.ed25519_VerifyBatch_zip215_indexed_dev(*good) == 0
    assert lib.ed25519_VerifyBatch_zip215_indexed_dev(p(res), p(dk), 4, p(di), p(ds), p(dm), 32, 0, seed, st) == 0
    torch.cuda.synchronize()
    assert int(res.cpu()[0, 0]) == 1
    for hole in (0, 1, 3, 4, 5, 8):                                               # a null pointer, the seed among them
        args = list(good)
        args[hole] = None
        assert lib.ed25519_VerifyBatch_zip215_indexed_dev(*args) != 0, hole
        assert lib.c25519_amd_last_error() != b""
    for n_key, n in ((0, 12), ((1 << 26) + 1, 12), (4, (1 << 26) + 1)):
        assert lib.ed25519_VerifyBatch_zip215_indexed_dev(p(res), p(dk), n_key, p(di), p(ds), p(dm), 32, n, seed, st) != 0, (n_key, n)
    assert lib.ed25519_VerifyBatch_zip215_indexed_ragged_dev(p(res), p(dk), 4, p(di), p(ds), p(dm), None, 12, seed, st) != 0
    assert lib.c25519_amd_verify_batch_indexed_point_dev(p(res), p(dk), 4, p(di), p(ds), p(dm), 32, 12, None, st) != 0
    assert lib.c25519_amd_verify_batch_indexed_point_dev(p(res), p(dk), 4, p(di), p(ds), p(dm), 32, 0, seed, st) != 0
    ok = C.c_int(-1)
    h = np.zeros((4, 64), np.uint8)
    hp = C.c_void_p(h.ctypes.data)
    assert lib.ed25519_VerifyBatch_zip215_indexed_batch(None, None, hp, 4, hp, hp, hp, 32, 4, None) != 0
    assert lib.ed25519_VerifyBatch_zip215_indexed_batch(C.byref(ok), None, None, 4, hp, hp, hp, 32, 4, None) != 0
    assert lib.ed25519_VerifyBatch_zip215_indexed_batch(C.byref(ok), None, hp, 4, None, hp, hp, 32, 4, None) != 0
    assert lib.ed25519_VerifyBatch_zip215_indexed_batch(C.byref(ok), None, hp, 0, hp, hp, hp, 32, 4, None) != 0
    assert lib.ed25519_VerifyBatch_zip215_indexed_ragged_batch(C.byref(ok), None, hp, 4, hp, hp, hp, None, 4, None) != 0
    assert ok.value == -1
    # one row and wz index entries per element, against two rows and wa + wz of them
    assert lib.ed25519_VerifyBatch_indexed_scratch_bytes(1 << 20, 256) < lib.ed25519_VerifyBatch_scratch_bytes(1 << 20) * 6 // 10


def test_two_host_threads_at_once(api, special):
    keys, idx, sig, msg, _ = make(api, special, 20000, 50, "random", 0x1DEB)
    bad = sig.copy()
    bad[12345, 33] ^= 1
    out, errors = {}, []

    def work(name, s, want):
        try:
            for j in range(4):
                got = api.ed25519_VerifyBatch_zip215_indexed(keys, idx, s, msg, seed=SEEDS[j % 3])
                assert got == want, (name, j, got)
            out[name] = True
        except Exception as e:  # noqa: BLE001
            errors.append((name, e))
        finally:
            _lib.load().c25519_amd_thread_release()

    with tunables(BATCH_EQ_INDEXED_MIN=1):
        threads = [threading.Thread(target=work, args=("good", sig, 1)), threading.Thread(target=work, args=("bad", bad, 0))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors and out == {"good": True, "bad": True}, errors
