"""GPU suite (MI355X): ZIP-215 batch verification, one equation per call -- ed25519_VerifyBatch_zip215_batch / _dev / _ragged_batch /
_ragged_dev and the hook c25519_amd_verify_batch_point_dev.  Expected results: the AND of the per-element ZIP-215 verdicts (the model
of tests/zip215_cases.py for the special rows, the reference's for honest and corrupted ones, as in tests/test_gpu_verify_zip215.py);
expected points: tests/batch_eq_model.py -- the slow model up to 64 elements, and at every size its closed form for rows whose S is
moved by a known delta (the host *_batch forms draw their seeds inside the library and cannot be steered: the closed form stays with
the *_dev forms and the hook).  Every case is a well-formed call."""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

import batch_eq_model as bm
import zip215_cases as zc
from curve25519_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 1024, 1025, 4096, 32769, 65537)
WIDTHS = (8, 10, 13)
ALL_WIDTHS = tuple(range(7, 14)) + (None,)                  # every width BATCH_EQ_WINDOW takes, and the default one
FIXED_SPECIAL = (1, 17, 62, 1023, 1024, 4095, 32768, 65536)  # where the valid fixture puts its first special rows
SEEDS = [bytes([29 * j + 3]) * 32 for j in range(3)]


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


def honest(api, n, seed, mlen=32):
    rng = np.random.default_rng(seed)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    return api.ed25519_SignMessage(priv, msg), pub, msg


def dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def result_dev(api, sig, pk, msg, seed):
    """ed25519_VerifyBatch_zip215_dev on device tensors -> int"""
    import torch
    res = torch.full((1, 1), -7, dtype=torch.int32, device=sig.device)
    api.ed25519_VerifyBatch_zip215_dev(res, sig, pk, msg, seed)
    return int(res.cpu()[0, 0])


def point_dev(api, sig, pk, msg, seed):
    import torch
    out = torch.zeros((1, 32), dtype=torch.uint8, device=sig.device)
    api.verify_batch_point_dev(out, sig, pk, msg, seed)
    return out.cpu().numpy()[0]


@pytest.fixture(scope="module")
def valid_rows(api, oracle):
    """65537 valid elements: honest signatures with every fourth (key, R) pair of the conformance grid (under 32-byte messages) and the
    24 torsion cases shuffled in; row 0 honest, row 1 and the rows around the sizes' edges special.  The special rows have the model's
    verdict 1, the honest ones the reference's."""
    n = SIZES[-1]
    sig, pk, msg = honest(api, n, 0xBA7C1)
    assert oracle.ed25519_verify(sig, pk, msg, threads=16).all()
    gsig, gpk, _ = (a[::4] for a in zc.conformance_grid())
    gmsg = np.random.default_rng(0xBA7C2).integers(0, 256, (len(gsig), 32), dtype=np.uint8)
    tsig, tpk, tmsg = zc.torsion()
    special = np.concatenate([gsig, tsig]), np.concatenate([gpk, tpk]), np.concatenate([gmsg, tmsg])
    assert zc.zip215_rule(*special).all()
    pos = np.random.default_rng(0xBA7C3).permutation(np.arange(1, n))[:len(special[0])]
    pos[:8] = FIXED_SPECIAL
    assert len(np.unique(pos)) == len(pos)
    sig[pos], pk[pos], msg[pos] = special
    return sig, pk, msg, pos


@pytest.fixture(scope="module")
def valid(valid_rows):
    """(sig, pk, msg) of valid_rows; its fourth entry: the special rows (every other row is honest and exactly valid under the
    reference's cofactorless equation)"""
    return valid_rows[:3]


@pytest.fixture(scope="module")
def valid_dev(valid):
    return dev(*valid)


# ---- the hook's point against the model -----------------------------------------------------------------------------------

@pytest.mark.parametrize("c", WIDTHS + (None,))
def test_hook_point_equals_the_model(api, valid, c):
    sig, pk, msg = valid
    for n in (64,) if c is None else (1, 2, 63):
        want, ok = bm.batch_point(sig[:n], pk[:n], msg[:n], SEEDS[0])
        with tunables(**({} if c is None else {"BATCH_EQ_WINDOW": c})):
            got = point_dev(api, *dev(sig[:n], pk[:n], msg[:n]), SEEDS[0])
        assert ok and np.array_equal(got, bm.encode(want)), (c, n)


def test_hook_leaves_rejected_elements_out(api, valid):
    sig, pk, msg = (a[:9].copy() for a in valid)
    sig[2, 32:] = np.frombuffer(bm.L.to_bytes(32, "little"), np.uint8)          # S = L
    pk[4] = bm.undecodable()
    sig[7, :32] = bm.undecodable()
    want, ok = bm.batch_point(sig, pk, msg, SEEDS[1])
    assert not ok
    d = dev(sig, pk, msg)
    assert np.array_equal(point_dev(api, *d, SEEDS[1]), bm.encode(want))
    with tunables(BATCH_EQ_MIN=1):
        assert result_dev(api, *d, SEEDS[1]) == 0
        for bad in (2, 4, 7):                                                     # each of the three alone
            keep = [i for i in range(9) if i not in {2, 4, 7} - {bad}]
            assert result_dev(api, *dev(sig[keep], pk[keep], msg[keep]), SEEDS[1]) == 0, bad


# ---- the equation at every size and width ---------------------------------------------------------------------------------

@pytest.mark.parametrize("c", WIDTHS)
def test_valid_batches_pass_and_one_bad_row_fails(api, valid_dev, c):
    sig, pk, msg = valid_dev
    rng = np.random.default_rng(0xBA7C5 + c)
    with tunables(BATCH_EQ_MIN=1, BATCH_EQ_WINDOW=c):
        for n in SIZES:
            for seed in SEEDS:
                assert result_dev(api, sig[:n], pk[:n], msg[:n], seed) == 1, (c, n)
                assert api.verify_batch_last_equation() == 1
            for row in sorted({0, n - 1, int(rng.integers(0, n))}):
                bad = sig[:n].clone()
                bad[row, 33] ^= 1                                                 # S off by 2^8: no rule accepts the element any more
                assert result_dev(api, bad, pk[:n], msg[:n], SEEDS[0]) == 0, (c, n, row)


@pytest.mark.parametrize("c", WIDTHS)
def test_cancelling_pair_inside_a_valid_batch_is_rejected(api, oracle, valid, c):
    sig, pk, msg = (a[:4096].copy() for a in valid)
    psig, ppk, pmsg = bm.cancelling_pair(oracle)
    assert zc.zip215_rule(psig, ppk, pmsg).tolist() == [0, 0]
    sig[[100, 3000]], pk[[100, 3000]], msg[[100, 3000]] = psig, ppk, pmsg
    with tunables(BATCH_EQ_MIN=1, BATCH_EQ_WINDOW=c):
        for seed in SEEDS:
            assert result_dev(api, *dev(sig, pk, msg), seed) == 0


@pytest.fixture(scope="module")
def million(api):
    """2^20 + 77 honest elements, signed on the device"""
    return honest(api, (1 << 20) + 77, 0xBA7C6)


def test_a_million_honest_elements_at_default_tunables(api, million):
    n = len(million[0])
    sig, pk, msg = dev(*million)
    assert result_dev(api, sig, pk, msg, SEEDS[2]) == 1
    sig[n // 3, 5] ^= 0x20
    assert result_dev(api, sig, pk, msg, SEEDS[2]) == 0


# ---- the closed form: exact points and steered accepts at every size ------------------------------------------------------

CLOSED_SIZES = tuple(n for n in SIZES if n >= 63)


def s_bytes(sig_row):
    """S of one signature as a device tensor of 32 bytes"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(sig_row[32:])).cuda()


@pytest.fixture(scope="module")
def shifted(valid_rows):
    """the valid fixture with S of every honest row moved by an odd 62-bit delta: (sig, rows, deltas, special rows ascending)"""
    sig, _, _, pos = valid_rows
    special = np.sort(pos)
    rows = np.setdiff1d(np.arange(len(sig)), special).tolist()
    deltas = bm.odd_deltas(len(rows), 0xBA7C9)
    return bm.shift_s(sig, rows, deltas), rows, deltas, special


@pytest.fixture(scope="module")
def shifted_dev(shifted, valid_dev):
    return dev(shifted[0])[0], valid_dev[1], valid_dev[2]


@pytest.fixture(scope="module")
def special_share(valid_rows):
    """seed -> {n: what the special rows below n add to the point of the first n elements}: the slow model, once per seed"""
    sig, pk, msg, pos = valid_rows
    special = np.sort(pos)
    return {seed: bm.subset_points(sig[special], pk[special], msg[special], seed, special, SIZES) for seed in SEEDS}


@pytest.fixture(scope="module")
def shift_sums(shifted):
    """seed -> the running sums of z_i d_i over the shifted rows: one pass over the challenges per seed, shared by every size"""
    _, rows, deltas, _ = shifted
    return {seed: bm.shift_sums(seed, rows, deltas) for seed in SEEDS}


@pytest.fixture(scope="module")
def rejected(valid_rows, shifted):
    """the shifted batch with three rejected honest rows (S = L, a key and an R that do not decode) inside every size's own stretch,
    away from its ends: (sig, pk, the shifted rows that stay, their deltas)"""
    _, pk, _, _ = valid_rows
    sig, rows, deltas, special = shifted
    sig, pk = sig.copy(), pk.copy()
    out, below = [], 0
    for n in CLOSED_SIZES:
        if n - below >= 8:
            for k in (1, 2, 3):
                row = below + (n - below) * k // 4
                while row in special or row in out:
                    row += 1
                out.append(row)
        below = n
    for j, row in enumerate(out):
        assert 0 < row < SIZES[-1] - 1 and row not in special
        if j % 3 == 0:
            sig[row, 32:] = np.frombuffer(bm.L.to_bytes(32, "little"), np.uint8)
        elif j % 3 == 1:
            pk[row] = bm.undecodable()
        else:
            sig[row, :32] = bm.undecodable()
    gone = set(out)
    kept = [(r, d) for r, d in zip(rows, deltas) if r not in gone]
    return sig, pk, [r for r, _ in kept], [d for _, d in kept]


def want_points(sums, share):
    return {(seed, n): bm.encode(bm.shifted_point(sums[seed], n, share[seed][n])) for seed in SEEDS for n in CLOSED_SIZES}


@pytest.fixture(scope="module")
def want_shifted(shift_sums, special_share):
    return want_points(shift_sums, special_share)


@pytest.fixture(scope="module")
def rejected_case(rejected, special_share, valid_dev):
    sig, pk, rows, deltas = rejected
    return dev(sig, pk) + (valid_dev[2],), want_points({seed: bm.shift_sums(seed, rows, deltas) for seed in SEEDS}, special_share)


@pytest.mark.parametrize("c", ALL_WIDTHS)
def test_shifted_rows_give_the_closed_form_point(api, shifted_dev, want_shifted, c):
    """every honest row's S moved by a known delta: T = [sum z_i d_i mod L]B plus the special rows' share, byte for byte, at every size
    from 63, for three seeds.  It holds only if element i gets z_i = SHA-512(seed || le64(i))[:16] and its own k_i, and every element
    is counted once."""
    sig, pk, msg = shifted_dev
    with tunables(**({} if c is None else {"BATCH_EQ_WINDOW": c})):
        for n in CLOSED_SIZES:
            for seed in SEEDS:
                got = point_dev(api, sig[:n], pk[:n], msg[:n], seed)
                assert np.array_equal(got, want_shifted[seed, n]), (c, n, seed[0])


@pytest.mark.parametrize("c", ALL_WIDTHS)
def test_shifted_rows_without_the_rejected_ones_give_the_closed_form_point(api, rejected_case, c):
    (sig, pk, msg), want = rejected_case
    with tunables(**({} if c is None else {"BATCH_EQ_WINDOW": c})):
        for n in CLOSED_SIZES:
            for seed in SEEDS:
                got = point_dev(api, sig[:n], pk[:n], msg[:n], seed)
                assert np.array_equal(got, want[seed, n]), (c, n, seed[0])
    with tunables(BATCH_EQ_MIN=1, **({} if c is None else {"BATCH_EQ_WINDOW": c})):
        assert result_dev(api, sig, pk, msg, SEEDS[0]) == 0


def steered_s(valid_rows, shift_sums, seed, n):
    """(row, S bytes on the device): the last row of the first n elements with the delta that makes sum z_i d_i = 0 mod L over them.
    The row may be a special one: moving its S adds [z d]B like any other row's."""
    row = n - 1
    delta = bm.steering_delta(seed, shift_sums[seed], n, row)
    return row, s_bytes(bm.shift_s(valid_rows[0][row:row + 1], [0], [delta])[0])


@pytest.mark.parametrize("c", WIDTHS)
def test_a_steered_batch_is_accepted_and_then_every_row_counts(api, valid_rows, shifted, shifted_dev, shift_sums, c):
    """Who knows the seed can choose one delta so that sum z_i d_i = 0 mod L: the equation then holds (T is an 8-torsion point: the
    special rows' share) although no honest row is valid, and the result is 1.  This is the defined behaviour of a batch rule under a
    KNOWN seed -- callers pass secret seeds -- and nothing to be fixed.  It holds only if every z_i and k_i is the right one; and from
    there, one more step in the S of any single row gives 0: every probed row is in the sums exactly once."""
    import torch
    host = shifted[0]
    sig, pk, msg = shifted_dev
    work = sig.clone()
    near_special = [r + d for r in FIXED_SPECIAL for d in (-1, 1)]
    with tunables(BATCH_EQ_MIN=1, BATCH_EQ_WINDOW=c):
        for k, n in enumerate(SIZES[1:]):
            seed = SEEDS[k % 3]
            last, steered = steered_s(valid_rows, shift_sums, seed, n)
            work[last, 32:] = steered
            assert result_dev(api, work[:n], pk[:n], msg[:n], seed) == 1, (c, n)
            assert api.verify_batch_last_equation() == 1
            runs = [r for _, r in bm.run_boundary_rows(n, 2 * n, max(256, 1 << c))]      # pts of batcheq_equation
            rows = bm.probe_rows(n, runs + near_special, seed=0xBA7CA + n + c)
            assert len(rows) >= min(n, 64)
            now = host[rows].copy()
            if last in rows:
                now[rows.index(last), 32:] = steered.cpu().numpy()
            bumped = dev(bm.shift_s(now, range(len(rows)), [1] * len(rows))[:, 32:])[0]
            res = torch.full((4 * len(rows), 1), -7, dtype=torch.int32, device="cuda")     # a result word is 16-byte aligned
            for j, row in enumerate(rows):
                keep = work[row, 32:].clone()
                work[row, 32:] = bumped[j]
                api.ed25519_VerifyBatch_zip215_dev(res[4 * j:4 * j + 1], work[:n], pk[:n], msg[:n], seed)
                work[row, 32:] = keep
            wrong = [rows[j] for j in np.flatnonzero(res.cpu().numpy()[::4, 0] != 0)]
            assert not wrong, (c, n, wrong)
            work[last, 32:] = sig[last, 32:]
    assert torch.equal(work, sig)


def test_the_per_element_path_rejects_the_steered_batch(api, valid_rows, shifted_dev, shift_sums):
    """the default BATCH_EQ_MIN: these sizes take the per-element path, which no steering passes"""
    sig, pk, msg = shifted_dev
    work = sig.clone()
    for k, n in enumerate(SIZES[1:]):
        seed = SEEDS[k % 3]
        last, steered = steered_s(valid_rows, shift_sums, seed, n)
        work[last, 32:] = steered
        assert result_dev(api, work[:n], pk[:n], msg[:n], seed) == 0, n
        assert api.verify_batch_last_equation() == 0
        work[last, 32:] = sig[last, 32:]


def test_a_steered_ragged_batch_is_accepted(api, oracle):
    """4096 messages of 0 .. 300 bytes (0, and the lengths at which the padding of SHA-512(R || A || M) takes one more block, among
    them) through ed25519_VerifyBatch_zip215_ragged_dev: every S moved, the last one steered -> 1; one more step in one row -> 0.  A k_i
    hashed over the wrong bytes leaves [z_i (k_i' - k_i)]A_i in T and cannot hide."""
    import torch
    n = 4096
    rng = np.random.default_rng(0xBA7CB)
    lens = rng.integers(0, 301, n)
    lens[:12] = [0, 47, 48, 175, 176, 300, 0, 1, 111, 112, 239, 240]
    lens[n - 3:] = [176, 0, 47]
    body = rng.integers(0, 256, (n, 300), dtype=np.uint8)
    messages = [body[i, :lens[i]].tobytes() for i in range(n)]
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    sig = api.ed25519_SignMessage_ragged(priv, messages)
    for length in np.unique(lens):                                               # exactly valid, each under its own length
        at = np.flatnonzero(lens == length)
        assert oracle.ed25519_verify(sig[at], pub[at], body[at, :length], threads=16).all(), length
    rows, deltas = list(range(n)), bm.odd_deltas(n, 0xBA7CC)
    deltas[n - 1] = bm.steering_delta(SEEDS[1], bm.shift_sums(SEEDS[1], rows, deltas), n, n - 1)
    steered = bm.shift_s(sig, rows, deltas)
    flat, offsets = api._ragged(messages)
    d_flat = torch.from_numpy(flat.reshape(-1, 1).copy()).cuda()
    d_off = torch.from_numpy(offsets.astype(np.int64).reshape(-1, 1)).cuda()
    d_pk, = dev(pub)
    res = torch.full((12, 1), -7, dtype=torch.int32, device="cuda")                # (a result word is 16-byte aligned)
    with tunables(BATCH_EQ_MIN=1):
        api.ed25519_VerifyBatch_zip215_ragged_dev(res[0:1], dev(steered)[0], d_pk, d_flat, d_off, SEEDS[1])
        assert api.verify_batch_last_equation() == 1
        api.ed25519_VerifyBatch_zip215_ragged_dev(res[4:5], dev(bm.shift_s(steered, [1234], [1]))[0], d_pk, d_flat, d_off, SEEDS[1])
    api.ed25519_VerifyBatch_zip215_ragged_dev(res[8:9], dev(steered)[0], d_pk, d_flat, d_off, SEEDS[1])      # the per-element path
    assert res.cpu().numpy()[::4, 0].tolist() == [1, 0, 0]


def test_a_million_shifted_elements_at_default_tunables(api, million):
    """2^20 + 77 elements signed on the device, every S moved: the exact point, then the steered accept, at the default width and
    threshold.  (The signatures are not checked against the reference first: an inexact one fails this test, it cannot hide a failure.)"""
    sig, pk, msg = million
    n = len(sig)
    rows, deltas = range(n), bm.odd_deltas(n, 0xBA7CD)
    sums = bm.shift_sums(SEEDS[2], rows, deltas)
    d_sig, d_pk, d_msg = dev(bm.shift_s(sig, rows, deltas), pk, msg)
    assert np.array_equal(point_dev(api, d_sig, d_pk, d_msg, SEEDS[2]), bm.encode(bm.shifted_point(sums, n)))
    row = n // 2 + 1
    d_sig[row, 32:] = s_bytes(bm.shift_s(sig[row:row + 1], [0], [bm.steering_delta(SEEDS[2], sums, n, row)])[0])
    assert result_dev(api, d_sig, d_pk, d_msg, SEEDS[2]) == 1
    assert api.verify_batch_last_equation() == 1
    d_sig[n - 300, 32] ^= 1                                                       # S one step off, far from the steered row
    assert result_dev(api, d_sig, d_pk, d_msg, SEEDS[2]) == 0


# ---- below BATCH_EQ_MIN ---------------------------------------------------------------------------------------------------

def test_below_the_threshold_the_per_element_path_gives_the_same_results(api, valid_dev):
    sig, pk, msg = valid_dev
    for n in (1, 63, 1025, 4096):
        bad = sig[:n].clone()
        bad[n // 2, 33] ^= 1
        with tunables(BATCH_EQ_MIN=n + 1):
            assert result_dev(api, sig[:n], pk[:n], msg[:n], SEEDS[0]) == 1
            assert api.verify_batch_last_equation() == 0
            assert result_dev(api, bad, pk[:n], msg[:n], SEEDS[0]) == 0
        with tunables(BATCH_EQ_MIN=n):
            assert result_dev(api, sig[:n], pk[:n], msg[:n], SEEDS[0]) == 1
            assert api.verify_batch_last_equation() == 1
        with tunables(BATCH_EQ_MIN=0):                                            # never
            assert result_dev(api, bad, pk[:n], msg[:n], SEEDS[0]) == 0
            assert api.verify_batch_last_equation() == 0


# ---- the host forms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 4096, (1 << 17) + 5])
def test_host_form_verdicts_and_null_arguments(api, valid, n):
    """(2^17 + 5: the call is cut into pieces, one equation each)"""
    sig, pk, msg = (np.concatenate([a, a, a])[:n] for a in valid) if n > len(valid[0]) else (a[:n] for a in valid)
    with tunables(BATCH_EQ_MIN=1):
        ok, verdict = api.ed25519_VerifyBatch_zip215(sig, pk, msg, seed=SEEDS[0], verdicts=True)
        assert ok == 1 and verdict.dtype == np.int32 and (verdict == 1).all()
        assert api.ed25519_VerifyBatch_zip215(sig, pk, msg, seed=SEEDS[1]) == 1   # a null verdict
        assert api.ed25519_VerifyBatch_zip215(sig, pk, msg) == 1                  # a null seed, twice
        assert api.ed25519_VerifyBatch_zip215(sig, pk, msg) == 1
        bad = sig.copy()
        bad[[0, n // 2, n - 1], 33] ^= 1
        bad[n // 3, 2] ^= 0x40
        ok, verdict = api.ed25519_VerifyBatch_zip215(bad, pk, msg, seed=SEEDS[0], verdicts=True)
        assert ok == 0 and np.array_equal(verdict, api.ed25519_VerifySignature_zip215(bad, pk, msg)) and (verdict == 0).sum() == 4
        assert api.ed25519_VerifyBatch_zip215(bad, pk, msg) == 0
        only_last = sig.copy()
        only_last[n - 1, 33] ^= 1                                                 # in the last piece of a call that is cut
        assert api.ed25519_VerifyBatch_zip215(only_last, pk, msg) == 0


def test_ragged_forms_equal_the_fixed_length_forms(api, valid):
    import torch
    n = 1500
    sig, pk, msg = (a[:n] for a in valid)
    messages = [m.tobytes() for m in msg]
    bad = sig.copy()
    bad[700, 33] ^= 1
    flat, offsets = api._ragged(messages)
    with tunables(BATCH_EQ_MIN=1):
        assert api.ed25519_VerifyBatch_zip215_ragged(sig, pk, messages, seed=SEEDS[0]) == 1 == api.ed25519_VerifyBatch_zip215(sig, pk, msg, seed=SEEDS[0])
        ok, verdict = api.ed25519_VerifyBatch_zip215_ragged(bad, pk, messages, verdicts=True)
        assert ok == 0 and np.array_equal(verdict, api.ed25519_VerifySignature_zip215(bad, pk, msg))
        d_flat = torch.from_numpy(flat.reshape(-1, 1).copy()).cuda()
        d_off = torch.from_numpy(offsets.astype(np.int64).reshape(-1, 1)).cuda()
        for s, want in ((sig, 1), (bad, 0)):
            res = torch.full((1, 1), -7, dtype=torch.int32, device="cuda")
            api.ed25519_VerifyBatch_zip215_ragged_dev(res, *dev(s, pk), d_flat, d_off, SEEDS[1])
            assert int(res.cpu()[0, 0]) == want
    # messages of different lengths: the hash sees each one's own bytes
    sig2, pk2, msg2 = honest(api, 40, 0xBA7C7, mlen=64)
    ragged = [msg2[i, :i + 1].tobytes() for i in range(40)]
    pub, priv = api.ed25519_CreateKeyPair(np.random.default_rng(0xBA7C8).integers(0, 256, (40, 32), dtype=np.uint8))
    rsig = api.ed25519_SignMessage_ragged(priv, ragged)
    with tunables(BATCH_EQ_MIN=1):
        assert api.ed25519_VerifyBatch_zip215_ragged(rsig, pub, ragged) == 1
        ragged[20] = ragged[20] + b"x"
        assert api.ed25519_VerifyBatch_zip215_ragged(rsig, pub, ragged) == 0


def test_empty_calls_and_argument_errors(api, valid_dev):
    import torch
    lib = _lib.load()
    sig, pk, msg = valid_dev
    assert api.ed25519_VerifyBatch_zip215(np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8), np.zeros((0, 0), np.uint8)) == 1
    res = torch.full((4, 1), -7, dtype=torch.int32, device="cuda")
    seed = C.create_string_buffer(SEEDS[0], 32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.ed25519_VerifyBatch_zip215_dev(p(res), p(sig), p(pk), p(msg), 32, 0, seed, st) == 0
    torch.cuda.synchronize()
    assert int(res.cpu()[0, 0]) == 1
    for args in ((None, p(sig), p(pk), p(msg), 32, 4, seed, st), (p(res), None, p(pk), p(msg), 32, 4, seed, st),
                 (p(res), p(sig), None, p(msg), 32, 4, seed, st), (p(res), p(sig), p(pk), None, 32, 4, seed, st),
                 (p(res), p(sig), p(pk), p(msg), 32, 4, None, st)):
        assert lib.ed25519_VerifyBatch_zip215_dev(*args) != 0
        assert lib.c25519_amd_last_error() != b""
    assert lib.ed25519_VerifyBatch_zip215_ragged_dev(p(res), p(sig), p(pk), p(msg), None, 4, seed, st) != 0
    assert lib.c25519_amd_verify_batch_point_dev(p(res), p(sig), p(pk), p(msg), 32, 4, None, st) != 0
    ok = C.c_int(-1)
    h = np.zeros((4, 64), np.uint8)
    hp = C.c_void_p(h.ctypes.data)
    assert lib.ed25519_VerifyBatch_zip215_batch(None, None, hp, hp, hp, 32, 4, None) != 0
    assert lib.ed25519_VerifyBatch_zip215_batch(C.byref(ok), None, None, hp, hp, 32, 4, None) != 0
    assert lib.ed25519_VerifyBatch_zip215_ragged_batch(C.byref(ok), None, hp, hp, hp, None, 4, None) != 0
    assert lib.ed25519_VerifyBatch_scratch_bytes(1 << 20) < lib.ed25519_VerifySignature_scratch_bytes(1 << 20) // 4


def test_two_host_threads_at_once(api, valid):
    sig, pk, msg = (a[:20000] for a in valid)
    bad = sig.copy()
    bad[12345, 33] ^= 1
    out, errors = {}, []

    def work(name, s, want):
        try:
            for j in range(4):
                got = api.ed25519_VerifyBatch_zip215(s, pk, msg, seed=SEEDS[j % 3])
                assert got == want, (name, j, got)
            out[name] = True
        except Exception as e:  # noqa: BLE001
            errors.append((name, e))
        finally:
            _lib.load().c25519_amd_thread_release()

    with tunables(BATCH_EQ_MIN=1):
        threads = [threading.Thread(target=work, args=("good", sig, 1)), threading.Thread(target=work, args=("bad", bad, 0))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not errors and out == {"good": True, "bad": True}, errors
