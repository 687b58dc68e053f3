"""GPU suite (MI355X): ed25519_Verify_Check_zip215_* -- the ZIP-215 verdict against Verify_Init contexts, one context or many.  For a
context that is Verify_Init's, element i's verdict is ed25519_VerifySignature_zip215's under the context's key bytes: expected verdicts
come from tests/check_zip215_model.py (big integers, a few hundred cases) and otherwise from ed25519_VerifySignature_zip215 on the
gathered keys.  ZIP215_CHECK_MIN = 0 forces the context path (walk, coset prep, shared inversion with the coset comparison); the
default sends small calls to the per-element kernels on the gathered keys."""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

import check_zip215_model as cm
import zip215_cases as zc
from curve25519_amd import _lib
from vectors import small_order_encodings

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@contextlib.contextmanager
def tunables(**kv):
    L = _lib.load()
    try:
        for k, v in kv.items():
            assert L.c25519_amd_tunable_set(k.encode(), v) == 0
        yield L
    finally:
        for k in kv:
            L.c25519_amd_tunable_set(k.encode(), -1)


def both_paths(fn):
    """fn() with the context path forced, and with the default tunable"""
    with tunables(ZIP215_CHECK_MIN=0):
        forced = fn()
    return forced, fn()


def by_key(api, pk):
    """(contexts of the distinct keys, index per element)"""
    keys, idx = np.unique(pk, axis=0, return_inverse=True)
    return api.ed25519_Verify_Init(np.ascontiguousarray(keys)), idx.reshape(-1).astype(np.uint32)


def keyset(api, k, seed):
    rng = np.random.default_rng(seed)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (k, 32), dtype=np.uint8))
    return pub, priv, api.ed25519_Verify_Init(pub)


def mixed(api, pub, priv, n, seed, mlen=24):
    """n triples over the keys: valid signatures, a corrupted signature / message in every 7th / 11th, every 13th index pointing at
    another key, and one wrong signature in the last quad"""
    rng = np.random.default_rng(seed)
    k = len(pub)
    idx = rng.integers(0, k, n).astype(np.uint32)
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    sig = api.ed25519_SignMessage(priv[idx], msg)
    sig[6::7, 40] ^= 4
    msg[3::11, 0] ^= 1
    if k > 1:
        idx[5::13] = (idx[5::13] + 1 + rng.integers(0, k - 1, len(idx[5::13]))) % k
    sig[n - 1 - (seed % min(n, 4)), 3] ^= 0x10
    return idx, sig, msg


def test_conformance_grid_through_contexts(api):
    """ZIP-215's 196 pairs of small-order encodings, the 14 encodings as 14 contexts: all valid, by the lane kernels and by default"""
    sig, pk, msg = zc.conformance_grid()
    encs = np.stack([np.frombuffer(e, np.uint8) for e, _ in small_order_encodings()])
    ctxs = api.ed25519_Verify_Init(encs)
    idx = np.repeat(np.arange(14, dtype=np.uint32), 14)
    assert np.array_equal(encs[idx], pk)
    want = cm.model_verdicts(sig, pk, msg)
    assert want.all() and len(want) == 196
    for got in both_paths(lambda: api.ed25519_Verify_Check_zip215_indexed(ctxs, idx, sig, msg)):
        assert np.array_equal(got, want)


def test_edge_sets_one_context_per_key(api, oracle):
    """tests/zip215_cases.py's edge set, the torsion and degenerate sets and the generated torsion-shift set (every encoding of R, flipped
    sign / y bits, S + 1, S + L, undecodable R and keys), one context per distinct key, lane path forced"""
    for name, (sig, pk, msg), model in (("torsion", zc.torsion(), True), ("generated", cm.generated_set()[:3], True),
                                        ("edge", zc.edge_set(oracle), False), ("degenerate", zc.degenerate()[:3], False)):
        ctxs, idx = by_key(api, pk)
        with tunables(ZIP215_CHECK_MIN=0):
            got = api.ed25519_Verify_Check_zip215_indexed(ctxs, idx, sig, msg)
        want = cm.model_verdicts(sig, pk, msg) if model else api.ed25519_VerifySignature_zip215(sig, pk, msg)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]])
        if not model:                                        # ... and the existing call agrees with the model on a sample
            s = np.arange(0, len(sig), max(1, len(sig) // 100))
            assert np.array_equal(want[s], cm.model_verdicts(sig[s], pk[s], msg[s])), name
        assert want.any() and (name == "torsion" or not want.all())


@pytest.mark.parametrize("k", [1, 3, 300])
def test_sizes_where_the_forms_change(api, k):
    """n = 1, 2, 1024, 1025, 1027, 4097 (tails in the shared inversion's groups above 1024) over k keys, forced and default"""
    pub, priv, ctxs = keyset(api, k, 0x2b00 + k)
    for n in (1, 2, 1024, 1025, 1027, 4097):
        idx, sig, msg = mixed(api, pub, priv, n, 0x2b10 + n)
        want = api.ed25519_VerifySignature_zip215(sig, pub[idx], msg)
        for got in both_paths(lambda: api.ed25519_Verify_Check_zip215_indexed(ctxs, idx, sig, msg)):
            assert np.array_equal(got, want), (k, n)
        assert not want[-4:].all() and (n < 8 or want.any())


def test_one_context(api):
    L = _lib.load()
    L.c25519_amd_verify_check_last_wide.restype = C.c_long
    pub, priv, ctxs = keyset(api, 1, 0x2b20)
    data = {n: mixed(api, pub, priv, n, 0x2b21 + n) for n in (1, 1025, 5000, 2049, 1500)}
    want = {n: api.ed25519_VerifySignature_zip215(s, pub[i], m) for n, (i, s, m) in data.items()}
    for n in (1, 1025, 5000):                               # the shared-table kernel (no comb: ONE_KEY_WIDE = 0), and the default
        with tunables(ONE_KEY_WIDE=0):
            for got in both_paths(lambda: api.ed25519_Verify_Check_zip215(ctxs[0], data[n][1], data[n][2])):
                assert np.array_equal(got, want[n]), n
            assert L.c25519_amd_verify_check_last_wide() == 0
    with tunables(ZIP215_CHECK_MIN=0, ONE_KEY_WIDE=2048):
        L.c25519_amd_thread_release()                        # no remembered comb
        got = api.ed25519_Verify_Check_zip215(ctxs[0], data[2049][1], data[2049][2])
        assert L.c25519_amd_verify_check_last_wide() == 1    # the comb is built and walked
        assert np.array_equal(got, want[2049])
        got = api.ed25519_Verify_Check_zip215(ctxs[0], data[1500][1], data[1500][2])
        assert L.c25519_amd_verify_check_last_wide() == 1    # below ONE_KEY_WIDE: the remembered comb, on the lane kernel
        assert np.array_equal(got, want[1500])
        # a key that does not decode: all 0, never the wide path
        bad_key = np.frombuffer(cm.undecodable_strings(1, 3)[0], np.uint8).reshape(1, 32)
        assert zc.zip215_decode(bad_key[0]) is None
        bad_ctx = api.ed25519_Verify_Init(bad_key)[0]
        got = api.ed25519_Verify_Check_zip215(bad_ctx, data[2049][1], data[2049][2])
        assert L.c25519_amd_verify_check_last_wide() == 0 and not got.any()
        # a mixed-order key and the eight torsion shifts of R: all accepted here, not by the plain call
        tsig, tpk, tmsg = zc.torsion()
        tctx = api.ed25519_Verify_Init(tpk[:1])[0]
        assert (tpk[:8] == tpk[0]).all()
        assert api.ed25519_Verify_Check_zip215(tctx, tsig[:8], tmsg[:8]).all()
        plain = api.ed25519_Verify_Check(tctx, tsig[:8], tmsg[:8])
        assert plain.any() and not plain.all()


def test_out_of_range_indices(api):
    """_dev: verdict 0 exactly where the index is >= n_ctx (also behind R = 0), right elsewhere; _batch: refused, verdict untouched"""
    import torch
    pub, priv, ctxs = keyset(api, 5, 0x2b30)
    dev = torch.device("cuda", 0)
    for n in (700, 5000):
        idx, sig, msg = mixed(api, pub, priv, n, 0x2b31 + n)
        bad = np.zeros(n, bool)
        bad[::10] = True
        idx_b = idx.copy()
        idx_b[bad] = np.where(np.arange(bad.sum()) % 2 == 0, 5, 0xFFFFFFFF)
        sig_b = sig.copy()
        sig_b[bad.nonzero()[0][::3], :32] = 0
        want = api.ed25519_VerifySignature_zip215(sig_b[~bad], pub[idx[~bad]], msg[~bad])
        t = [torch.from_numpy(a).to(dev) for a in (ctxs, idx_b.view(np.int32).reshape(n, 1), sig_b, msg)]

        def run():
            d_v = torch.full((n, 1), -1, dtype=torch.int32, device=dev)
            api.ed25519_Verify_Check_zip215_indexed_dev(d_v, *t)
            torch.cuda.synchronize()
            return d_v.cpu().numpy().reshape(-1)

        for v in both_paths(run):
            assert not v[bad].any() and np.array_equal(v[~bad], want), n
    idx, sig, msg = mixed(api, pub, priv, 300, 0x2b32)
    idx[123] = 5
    out = np.full(300, 7, np.int32)
    L = _lib.load()
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    for mn in (0, -1):
        with tunables(ZIP215_CHECK_MIN=mn):
            assert L.ed25519_Verify_Check_zip215_indexed_batch(p(out), p(ctxs), 5, p(idx), p(sig), p(msg), msg.shape[1], 300) != 0
            assert (out == 7).all()
            with pytest.raises(_lib.EngineError):
                api.ed25519_Verify_Check_zip215_indexed(ctxs, idx, sig, msg)
            assert L.ed25519_Verify_Check_zip215_indexed_batch(p(out), p(ctxs), 0, p(idx), p(sig), p(msg), msg.shape[1], 300) != 0
            assert L.ed25519_Verify_Check_zip215_indexed_batch(p(out), p(ctxs), 5, p(idx), p(sig), p(msg), msg.shape[1], 0) == 0
            assert (out == 7).all()


def test_ragged_messages(api):
    """message lengths 0..200, the host form and the device form, forced and default"""
    import torch
    rng = np.random.default_rng(0x2b40)
    pub, priv, ctxs = keyset(api, 23, 0x2b41)
    n = 1500
    idx = rng.integers(0, 23, n).astype(np.uint32)
    messages = [rng.integers(0, 256, int(rng.integers(0, 201)), dtype=np.uint8).tobytes() for _ in range(n)]
    messages[0], messages[1] = b"", bytes(200)
    sig = api.ed25519_SignMessage_ragged(priv[idx], messages)
    sig[::9, 33] ^= 1
    idx[4::17] = (idx[4::17] + 1) % 23
    want = api.ed25519_VerifySignature_zip215_ragged(sig, pub[idx], messages)
    assert 0.5 < want.mean() < 0.95
    for got in both_paths(lambda: api.ed25519_Verify_Check_zip215_indexed_ragged(ctxs, idx, sig, messages)):
        assert np.array_equal(got, want)
    dev = torch.device("cuda", 0)
    lens = np.array([len(m) for m in messages], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).reshape(-1, 1)
    flat = np.frombuffer(b"".join(messages) + b"\0", np.uint8).reshape(-1, 1).copy()
    t = [torch.from_numpy(a).to(dev) for a in (ctxs, idx.view(np.int32).reshape(n, 1), sig, flat, offsets)]

    def run():
        d_v = torch.full((n, 1), -1, dtype=torch.int32, device=dev)
        api.ed25519_Verify_Check_zip215_indexed_ragged_dev(d_v, *t)
        torch.cuda.synchronize()
        return d_v.cpu().numpy().reshape(-1)

    for got in both_paths(run):
        assert np.array_equal(got, want)


def test_host_call_of_more_than_one_piece(api):
    n = (1 << 17) + 3
    pub, priv, ctxs = keyset(api, 300, 0x2b50)
    idx, sig, msg = mixed(api, pub, priv, n, 0x2b51, mlen=16)
    want = api.ed25519_VerifySignature_zip215(sig, pub[idx], msg)
    assert 0.5 < want.mean() < 0.95
    for got in both_paths(lambda: api.ed25519_Verify_Check_zip215_indexed(ctxs, idx, sig, msg)):
        assert np.array_equal(got, want)


def test_two_threads(api):
    """two host threads at once, each with its own contexts, one forced onto the context path by size"""
    sets = [keyset(api, 11 + 6 * t, 0x2b60 + t) for t in range(2)]
    jobs = [mixed(api, pub, priv, 9000, 0x2b62 + t) for t, (pub, priv, _) in enumerate(sets)]
    refs = [api.ed25519_VerifySignature_zip215(jobs[t][1], sets[t][0][jobs[t][0]], jobs[t][2]) for t in range(2)]
    results, errors = [[], []], []

    def work(t):
        try:
            for _ in range(3):
                results[t].append(api.ed25519_Verify_Check_zip215_indexed(sets[t][2], *jobs[t]))
                results[t].append(api.ed25519_Verify_Check_zip215(sets[t][2][0], jobs[t][1][:3000], jobs[t][2][:3000]))
            _lib.load().c25519_amd_thread_release()
        except Exception as e:                      # noqa: BLE001 (reported below)
            errors.append(e)

    with tunables(ZIP215_CHECK_MIN=0):
        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
    assert not errors, errors
    for t in range(2):
        one = api.ed25519_VerifySignature_zip215(jobs[t][1][:3000], np.repeat(sets[t][0][:1], 3000, axis=0), jobs[t][2][:3000])
        assert len(results[t]) == 6
        assert all(np.array_equal(r, refs[t]) for r in results[t][0::2]) and all(np.array_equal(r, one) for r in results[t][1::2])


def test_plain_calls_unchanged_on_the_same_thread_and_context(api):
    """the plain calls after a ZIP-215 call that built the comb for the same context bytes: plain verdicts, and the kept comb is used"""
    L = _lib.load()
    L.c25519_amd_verify_check_last_wide.restype = C.c_long
    tsig, tpk, tmsg = zc.torsion()
    pub, priv, ctxs = keyset(api, 4, 0x2b70)
    idx, sig, msg = mixed(api, pub[:1], priv[:1], 2049, 0x2b71, mlen=32)
    sig[:8], msg[:8] = tsig[:8], tmsg[:8]                    # eight rows that are not this key's: 0 under either rule
    with tunables(ZIP215_CHECK_MIN=0, ONE_KEY_WIDE=2048):
        L.c25519_amd_thread_release()
        z = api.ed25519_Verify_Check_zip215(ctxs[0], sig, msg)
        assert L.c25519_amd_verify_check_last_wide() == 1
        plain = api.ed25519_Verify_Check(ctxs[0], sig, msg)
        assert L.c25519_amd_verify_check_last_wide() == 1
        assert np.array_equal(plain, api.ed25519_VerifySignature(sig, np.repeat(pub[:1], 2049, axis=0), msg))
        assert np.array_equal(z, api.ed25519_VerifySignature_zip215(sig, np.repeat(pub[:1], 2049, axis=0), msg))
        # many contexts, one of them a mixed-order key: the ZIP-215 call accepts its eight shifts, the plain call after it does not
        all_ctx = np.concatenate([ctxs, api.ed25519_Verify_Init(tpk[:1])])
        idx4, sig4, msg4 = mixed(api, pub, priv, 3000, 0x2b72, mlen=32)
        idx4[:8], sig4[:8], msg4[:8] = 4, tsig[:8], tmsg[:8]
        keys = np.concatenate([pub, tpk[:1]])[idx4]
        zi = api.ed25519_Verify_Check_zip215_indexed(all_ctx, idx4, sig4, msg4)
        pi = api.ed25519_Verify_Check_indexed(all_ctx, idx4, sig4, msg4)
        assert np.array_equal(zi, api.ed25519_VerifySignature_zip215(sig4, keys, msg4)) and zi[:8].all()
        assert np.array_equal(pi, api.ed25519_VerifySignature(sig4, keys, msg4)) and not pi[:8].all()
