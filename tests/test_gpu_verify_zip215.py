"""GPU suite (MI355X): the ZIP-215 verification calls -- ed25519_VerifySignature_zip215_batch / _dev / _ragged_batch / _ragged_dev.
Expected verdicts: the rule in Python big integers (tests/zip215_cases.py).  Every dispatch shape is covered: per wave (n <= 1024),
quads (1025 .. 32768), one lane per element, and the cofactored fallback under a low lattice cap; a key off the curve must reach no
other kernel."""
import contextlib
import threading

import numpy as np
import pytest

import strict_cases as sc
import zip215_cases as zc
from curve25519_amd import _lib
from vectors import L

pytestmark = pytest.mark.gpu

SIZES = (1, 1024, 1025, 4096, 32768, 32769, 65537)
PATHS = {"wave": (), "quad": (("COOP_MAX", 0), ("QUAD_MIN", 0)), "lane": (("COOP_MAX", 0), ("QUAD_MAX", 0))}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def honest(api, n, seed, mlen=32):
    rng = np.random.default_rng(seed)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    return api.ed25519_SignMessage(priv, msg), pub, msg


@contextlib.contextmanager
def tunables(pairs):
    """the tunables of `pairs` set, and restored however the block leaves"""
    with contextlib.ExitStack() as st:
        for k, v in pairs:
            st.enter_context(_lib.tunable(k, v))
        yield


def zip215_on(api, path, *args):
    with tunables(PATHS[path]):
        return api.ed25519_VerifySignature_zip215(*args)


@pytest.fixture(scope="module")
def edges(oracle):
    sig, pk, msg = zc.edge_set(oracle)
    return sig, pk, msg, zc.zip215_rule(sig, pk, msg)


@pytest.fixture(scope="module")
def mixed(api, oracle, edges):
    """65537 elements, shuffled: honest and corrupted signatures, the edge set, the conformance grid's 196 (key, R) pairs under
    32-byte messages; row 0 honest.  (sig, pk, msg, ZIP-215 verdicts).  The edge and grid rows get the model's verdict.  The honest
    and corrupted rows get the reference's: their keys are a*B, canonical, with S < L, where the cofactored and the cofactorless
    equation differ only if R is off by a torsion point, which flipping a bit does not produce; a sample of them is put to the model."""
    n = SIZES[-1]
    sig, pk, msg = honest(api, n, 0x215A1)
    sig[5::101, 7] ^= 0x10
    sig[9::103, 40] ^= 0x04
    want = oracle.ed25519_verify(sig, pk, msg, threads=16)
    esig, epk, emsg, ewant = edges
    gsig, gpk, _ = zc.conformance_grid()
    gmsg = np.random.default_rng(0x215A2).integers(0, 256, (len(gsig), 32), dtype=np.uint8)
    gwant = zc.zip215_rule(gsig, gpk, gmsg)
    assert gwant.all()
    special = np.concatenate([esig, gsig]), np.concatenate([epk, gpk]), np.concatenate([emsg, gmsg]), np.concatenate([ewant, gwant])
    rng = np.random.default_rng(0x215A3)
    pos = rng.permutation(np.arange(1, n))[:len(special[0])]                     # shuffled in, row 0 stays honest
    pos[:8] = [1023, 1024, 4095, 32767, 32768, 65536, 2, 1]                      # ... and the dispatch edges get special rows
    assert len(np.unique(pos)) == len(pos)
    sig[pos], pk[pos], msg[pos], want[pos] = special
    rest = np.setdiff1d(np.arange(n), pos)
    sample = np.concatenate([rest[:16], np.intersect1d(rest, np.arange(5, n, 101))[:16], np.intersect1d(rest, np.arange(9, n, 103))[:16]])
    assert np.array_equal(zc.zip215_rule(sig[sample], pk[sample], msg[sample]), want[sample])
    return sig, pk, msg, want


@pytest.mark.parametrize("knob", [None, ("QUAD_MAX", 0), ("COOP_MAX", 0), ("VERIFY_LAT_CAP_BITS", 100)])
def test_zip215_verdicts_equal_the_model(api, mixed, knob):
    sig, pk, msg, want = mixed
    assert want[0] == 1 and want.sum() > SIZES[-1] // 2 and (want == 0).sum() > 700
    for n in SIZES:
        with tunables([knob] if knob else []):
            got = api.ed25519_VerifySignature_zip215(sig[:n], pk[:n], msg[:n])
        assert np.array_equal(got, want[:n]), (knob, n, np.nonzero(got != want[:n])[0][:10])
    if knob == ("VERIFY_LAT_CAP_BITS", 100):
        with tunables([knob]):
            api.ed25519_VerifySignature_zip215(sig, pk, msg)
            assert _lib.load().c25519_amd_verify_last_slow_elements() > 1000     # over-long vectors did take the cofactored fallback


@pytest.mark.parametrize("path", sorted(PATHS))
def test_edge_set_alone_on_every_shape(api, edges, path):
    sig, pk, msg, want = edges
    got = zip215_on(api, path, sig, pk, msg)
    assert np.array_equal(got, want), (path, np.nonzero(got != want)[0][:10])
    assert want.sum() >= 64 and (want == 0).sum() >= 64
    with tunables(PATHS[path] + (("VERIFY_LAT_CAP_BITS", 100),)):
        got = api.ed25519_VerifySignature_zip215(sig, pk, msg)
        assert _lib.load().c25519_amd_verify_last_slow_elements() > 0
    assert np.array_equal(got, want), (path, "fallback", np.nonzero(got != want)[0][:10])


@pytest.mark.parametrize("path", sorted(PATHS))
def test_conformance_grid_is_accepted_on_every_shape(api, path):
    sig, pk, msg = zc.conformance_grid()
    assert len(sig) == 196 and msg[0].tobytes() == b"Zcash"
    assert zip215_on(api, path, sig, pk, msg).all()
    assert _lib.load().c25519_amd_verify_last_slow_elements() == 0
    assert not api.ed25519_VerifySignature_strict(sig, pk, msg).any()           # the strict calls reject every one of them


@pytest.mark.parametrize("path", sorted(PATHS))
def test_torsion_and_s_plus_l_differ_from_the_plain_call(api, oracle, path):
    sig, pk, msg = zc.torsion()
    assert zip215_on(api, path, sig, pk, msg).all()
    assert 0 < api.ed25519_VerifySignature(sig, pk, msg).sum() < len(sig)
    hsig, hpk, hmsg = honest(api, 64, 0x215A4)
    lsig, _ = sc.hostile(hsig, hpk, "s_plus_l")
    assert zip215_on(api, path, hsig, hpk, hmsg).all() and not zip215_on(api, path, lsig, hpk, hmsg).any()
    assert api.ed25519_VerifySignature(lsig, hpk, hmsg).all()


def test_degenerate_set(api):
    sig, pk, msg, _ = zc.degenerate()
    want = zc.zip215_rule(sig, pk, msg)
    assert want.sum() == 388
    for path in sorted(PATHS):
        assert np.array_equal(zip215_on(api, path, sig, pk, msg), want), path


@pytest.mark.parametrize("n", [1000, 4096, 65536])
def test_off_curve_keys_reach_no_other_kernel(api, n):
    sig, pk, msg = honest(api, n, 0x215A5)
    hsig, hpk = sc.hostile(sig, pk, "offcurve")
    got = api.ed25519_VerifySignature_zip215(hsig, hpk, msg)
    assert _lib.load().c25519_amd_verify_last_slow_elements() == 0
    assert not got[1::2].any() and got[0::2].all()
    rsig = sig.copy()
    rsig[1::2, :32] = hpk[1]                                                     # ... and the same string as R
    got = api.ed25519_VerifySignature_zip215(rsig, pk, msg)
    assert _lib.load().c25519_amd_verify_last_slow_elements() == 0
    assert not got[1::2].any() and got[0::2].all()


def test_ragged_forms_equal_the_fixed_length_ones(api, edges):
    import torch
    esig, epk, emsg, ewant = edges
    rng = np.random.default_rng(0x215A6)
    for n in (700, 5000, 40000):
        pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (n, 32), dtype=np.uint8))
        lens = rng.integers(0, 300, n)
        lens[:4] = [0, 129, 0, 299]
        msgs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
        sig = api.ed25519_SignMessage_ragged(priv, msgs)
        sig[7::13, 33] ^= 0x20
        # the edge set keeps its 32-byte messages; every other row is compared with the fixed-length call of its own length class
        k = min(len(esig), (n - 6) // 2)
        pos = np.arange(5, 5 + 2 * k, 2)
        sig[pos], pub[pos] = esig[:k], epk[:k]
        for j, p in enumerate(pos):
            msgs[p] = emsg[j].tobytes()
            lens[p] = 32
        got = api.ed25519_VerifySignature_zip215_ragged(sig, pub, msgs)
        assert np.array_equal(got[pos], ewant[:k]), n
        for length in (0, 32, 129, 299):
            idx = np.nonzero(lens == length)[0]
            assert len(idx) > 0
            fixed = np.stack([np.frombuffer(msgs[i], np.uint8) for i in idx]).reshape(len(idx), length)
            assert np.array_equal(got[idx], api.ed25519_VerifySignature_zip215(sig[idx], pub[idx], fixed)), (n, length)
        plain = api.ed25519_VerifySignature_ragged(sig, pub, msgs)
        rest = np.setdiff1d(np.arange(n), pos)
        assert np.array_equal(got[rest], plain[rest]) and got[rest].sum() > len(rest) // 2    # honest keys: the two rules agree
        flat = np.frombuffer(b"".join(msgs), np.uint8)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        d = [torch.from_numpy(a.copy()).cuda() for a in (sig, pub, flat, offs)]
        out = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        rc = _lib.load().ed25519_VerifySignature_zip215_ragged_dev(out.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                                  d[3].data_ptr(), n, st)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got), n


def test_batch_in_pieces_and_two_threads(api, mixed):
    sig, pk, msg, want = mixed
    reps = 4                                                         # 262148 rows: the host pipeline cuts them into pieces
    big = [np.concatenate([a] * reps) for a in (sig, pk, msg)]
    assert np.array_equal(api.ed25519_VerifySignature_zip215(*big), np.concatenate([want] * reps))
    out, errs = {}, []

    def work(k):
        try:
            lo = 9000 * k
            for _ in range(3):
                out[k] = api.ed25519_VerifySignature_zip215(sig[lo:lo + 30000], pk[lo:lo + 30000], msg[lo:lo + 30000])
        except Exception as e:                                        # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for k in range(2):
        assert np.array_equal(out[k], want[9000 * k:9000 * k + 30000]), k


def test_device_form_on_two_streams_of_one_thread(api, mixed):
    """calls of one, of per-wave, quad and lane size in turn on two streams: every call gets its own verdicts (and a call of one its
    completion word)"""
    import torch
    sig, pk, msg, want = mixed
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()                # noqa: E731
    cuts = [(0, 1), (1, 2), (0, 700), (700, 5700), (0, 40000), (1024, 1025)]
    cases = [(dev(sig[a:b]), dev(pk[a:b]), dev(msg[a:b]), want[a:b]) for a, b in cuts]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(6):
        outs = []
        for k, (s, p, m, _) in enumerate(cases):
            with torch.cuda.stream(streams[(k + rep) % 2]):
                out = torch.full((s.shape[0], 1), 7, dtype=torch.int32, device="cuda")
                api.ed25519_VerifySignature_zip215_dev(out, s, p, m)
                outs.append(out)
        torch.cuda.synchronize()
        for k, (out, case) in enumerate(zip(outs, cases)):
            assert np.array_equal(out.cpu().numpy()[:, 0], case[3]), (rep, k)


def test_honest_inputs_all_three_device_calls_agree(api):
    import torch
    for n in (1, 1024, 4096, 65536):
        sig, pk, msg = honest(api, n, 0x215A7 + n)
        sig[3::17, 50] ^= 1
        t = [torch.from_numpy(a).cuda() for a in (sig, pk, msg)]
        plain = torch.empty((n, 1), dtype=torch.int32, device="cuda")
        strict = torch.full((n, 1), 7, dtype=torch.int32, device="cuda")
        zip215 = torch.full((n, 1), 7, dtype=torch.int32, device="cuda")
        api.ed25519_VerifySignature_dev(plain, *t)
        api.ed25519_VerifySignature_strict_dev(strict, *t)
        api.ed25519_VerifySignature_zip215_dev(zip215, *t)
        assert torch.equal(plain, strict) and torch.equal(plain, zip215), n
        assert int(plain.sum()) == n - len(range(3, n, 17))


def test_argument_rules(api):
    lib = _lib.load()
    sig, pk, msg = honest(api, 4, 0x215A8)
    out = np.full(4, 7, np.int32)
    p = lambda a: a.ctypes.data                                                  # noqa: E731
    assert lib.ed25519_VerifySignature_zip215_batch(p(out), p(sig), p(pk), p(msg), 32, 0) == 0 and (out == 7).all()
    assert lib.ed25519_VerifySignature_zip215_batch(None, p(sig), p(pk), p(msg), 32, 4) != 0
    assert lib.ed25519_VerifySignature_zip215_batch(p(out), None, p(pk), p(msg), 32, 4) != 0
    assert lib.ed25519_VerifySignature_zip215_batch(p(out), p(sig), None, p(msg), 32, 4) != 0
    assert lib.ed25519_VerifySignature_zip215_batch(p(out), p(sig), p(pk), None, 32, 4) != 0
    assert lib.ed25519_VerifySignature_zip215_batch(p(out), p(sig), p(pk), None, 0, 4) == 0       # empty messages need no pointer
    offs = np.zeros(5, np.uint64)
    assert lib.ed25519_VerifySignature_zip215_ragged_batch(p(out), p(sig), p(pk), None, None, 4) != 0
    assert lib.ed25519_VerifySignature_zip215_ragged_batch(p(out), p(sig), p(pk), None, p(offs), 0) == 0
    assert lib.ed25519_VerifySignature_zip215_dev(None, None, None, None, 0, 4, None) != 0
    assert lib.ed25519_VerifySignature_zip215_ragged_dev(None, None, None, None, None, 4, None) != 0
    assert api.ed25519_VerifySignature_zip215(sig, pk, msg).all()
