"""GPU suite (MI355X): curve25519_dh_Peer_Init_* and curve25519_dh_CreateSharedKey_indexed_* -- n secrets against n_ctx peer contexts
in one call.  Every output and every clamped secret must equal what curve25519_dh_CreateSharedKey_dev gives with the keys gathered
(pk[ctx_index[i]]), for every peer class mixed into one call; c25519_amd_x25519_indexed_last_ladder_elements must show that the
contexts' rows really decided the eligible elements above PEER_INDEXED_MIN (otherwise a gather-then-ladder implementation would
pass every parity check)."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import one_peer_cases as cases
import peer_ctx_model as model
from curve25519_amd import _lib, synth

pytestmark = pytest.mark.gpu

MIN = 2049                            # the default PEER_INDEXED_MIN (test_threshold_default pins it)
SIZES = (1, 2, 65, 3584, 3585, MIN - 1, MIN + 1, (1 << 16) + 1, 1 << 20)
SPECIAL = ("twist2", "small2", "small5", "minus_one0", "bit255_on", "bit255_off")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def peer_keys(api, k, seed):
    """k peer keys: public keys of random secrets with the special classes (twist, small order, u = -1, bit 255) spread among them"""
    pk, _ = api.curve25519_dh_CalculatePublicKey(synth.random_bytes((k, 32), 0x0f0000 + seed))
    fixed = dict(cases.fixed_peers())
    for j, name in enumerate(SPECIAL):
        if j * 7 < k:
            pk[j * 7] = np.frombuffer(fixed[name], np.uint8)
    return pk


def init_dev(api, pk):
    import torch
    d_ctx = torch.empty((len(pk), model.CTX_SIZE), dtype=torch.uint8, device=dev())
    api.curve25519_dh_Peer_Init_dev(d_ctx, to_dev(pk))
    return d_ctx


def indexed_dev(api, d_ctx, idx, sk):
    import torch
    d_sk = to_dev(sk)
    d_out = torch.empty_like(d_sk)
    api.curve25519_dh_CreateSharedKey_indexed_dev(d_out, d_ctx, to_dev(np.asarray(idx, np.uint32).view(np.int32).reshape(-1, 1)), d_sk)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_sk.cpu().numpy()


def ladder_dev(api, keys, sk):
    import torch
    d_sk = to_dev(sk)
    d_out = torch.empty_like(d_sk)
    api.curve25519_dh_CreateSharedKey_dev(d_out, to_dev(keys), d_sk)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_sk.cpu().numpy()


def indices(k, n, seed, order):
    idx = np.random.default_rng(seed).integers(0, k, n).astype(np.uint32)
    return np.sort(idx) if order == "sorted" else idx


def last_ladder():
    return _lib.load().c25519_amd_x25519_indexed_last_ladder_elements()


def test_threshold_default(api):
    """with PEER_INDEXED_MIN unset, a call of MIN secrets walks the contexts' rows and one of MIN - 1 runs the ladder"""
    assert _lib.load().c25519_amd_tunable_get(b"PEER_INDEXED_MIN") == -1
    pk, _ = api.curve25519_dh_CalculatePublicKey(synth.random_bytes((16, 32), 0x0f08))
    d_ctx = init_dev(api, pk)
    sk = synth.random_bytes((MIN, 32), 0x0f09)
    idx = indices(16, MIN, 0x0a, "random")
    indexed_dev(api, d_ctx, idx, sk)
    assert last_ladder() == 0
    indexed_dev(api, d_ctx, idx[:-1], sk[:-1])
    assert last_ladder() == MIN - 1


def test_context_bytes(api):
    """Peer_Init_batch and Peer_Init_dev give identical bytes, and both equal the big-integer model, for every class"""
    import torch
    pk = np.array([np.frombuffer(p, np.uint8) for _, p in cases.fixed_peers() + cases.random_peers(16, 0x0f60)])
    host = api.curve25519_dh_Peer_Init(pk)
    d = init_dev(api, pk)
    torch.cuda.synchronize()
    assert np.array_equal(host, d.cpu().numpy())
    assert np.array_equal(host, model.contexts(pk))
    big = peer_keys(api, 70_000, 1)                 # several k_x25519_peer_init chunks
    d = init_dev(api, big)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(got, api.curve25519_dh_Peer_Init(big))
    for j in (0, 7, 14, 21, 28, 35, 40_000, 69_999):
        assert np.array_equal(got[j], np.frombuffer(model.context(big[j].tobytes()), np.uint8)), j


@pytest.mark.parametrize("k", [1, 37, 4096, 70_000])
def test_parity_with_the_ladder(api, k):
    """every size where the dispatch changes, random and sorted indices, the special classes mixed in: bytes and clamped secrets
    equal CreateSharedKey_dev on the gathered keys"""
    pk = peer_keys(api, k, k)
    d_ctx = init_dev(api, pk)
    for j, n in enumerate(SIZES):
        for order in ("random", "sorted"):
            if n == 1 << 20 and order == "sorted" and k != 4096:
                continue
            idx = indices(k, n, 16 * j + len(order), order)
            sk = synth.random_bytes((n, 32), 0x0f1000 + 64 * j + k % 61)
            got, got_sk = indexed_dev(api, d_ctx, idx, sk)
            exp, exp_sk = ladder_dev(api, pk[idx], sk)
            assert np.array_equal(got, exp), (k, n, order)
            assert np.array_equal(got_sk, exp_sk), (k, n, order)


def test_digest_at_2_20(api):
    """2^20 secrets against 4096 contexts: SHA-256 of the output equals that of CreateSharedKey_dev on the gathered keys"""
    n, k = 1 << 20, 4096
    pk = peer_keys(api, k, 0x20)
    d_ctx = init_dev(api, pk)
    idx = indices(k, n, 0x21, "random")
    sk = synth.random_bytes((n, 32), 0x0f2000)
    got, _ = indexed_dev(api, d_ctx, idx, sk)
    exp, _ = ladder_dev(api, pk[idx], sk)
    assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(exp.tobytes()).hexdigest()


def test_path_hook(api):
    """0 above the crossover with every context eligible; t with t elements on twist contexts; n below the crossover"""
    pk, _ = api.curve25519_dh_CalculatePublicKey(synth.random_bytes((64, 32), 0x0f30))
    pk[5] = np.frombuffer(cases.to_bytes(cases.TWIST[0]), np.uint8)
    d_ctx = init_dev(api, pk)
    L = _lib.load()
    L.c25519_amd_thread_release()
    assert last_ladder() == -1
    n = MIN + 5
    idx = indices(64, n, 0x31, "random")
    idx[idx == 5] = 6
    sk = synth.random_bytes((n, 32), 0x0f31)
    got, _ = indexed_dev(api, d_ctx, idx, sk)
    assert last_ladder() == 0
    t = 123
    idx[np.random.default_rng(0x32).choice(n, t, replace=False)] = 5
    got, _ = indexed_dev(api, d_ctx, idx, sk)
    assert last_ladder() == t
    assert np.array_equal(got, ladder_dev(api, pk[idx], sk)[0])
    for m in (1, 1000, MIN - 1):
        indexed_dev(api, d_ctx, idx[:m], sk[:m])
        assert last_ladder() == m
    with _lib.tunable("PEER_INDEXED_MIN", 0):
        got, _ = indexed_dev(api, d_ctx, idx[:100], sk[:100])
        assert last_ladder() == int((idx[:100] == 5).sum())
        assert np.array_equal(got, ladder_dev(api, pk[idx[:100]], sk[:100])[0])


def test_bad_indices_on_dev(api):
    """indices n_ctx .. n_ctx + 3 into an allocation that holds four sentinel contexts beyond n_ctx: 32 zero bytes and clamped
    secrets there, the ladder's bytes elsewhere, below and above the crossover"""
    k = 40
    pk = peer_keys(api, k + 4, 0x40)
    d_all = init_dev(api, pk)
    d_ctx = d_all[:k]
    for n in (700, MIN + 9):
        idx = indices(k, n, 0x41 + n, "random")
        bad = np.zeros(n, bool)
        bad[::9] = True
        idx[bad] = k + np.arange(bad.sum()) % 4
        sk = synth.random_bytes((n, 32), 0x0f40 + n)
        got, got_sk = indexed_dev(api, d_ctx, idx, sk)
        exp, exp_sk = ladder_dev(api, pk[np.where(bad, 0, idx)], sk)
        assert not got[bad].any(), n
        assert np.array_equal(got[~bad], exp[~bad]), n
        assert np.array_equal(got_sk, exp_sk), n


def test_host_refusals(api):
    """_batch: an out-of-range index refuses the call with shared and sk untouched; n_ctx = 0 and null pointers are argument
    errors; n = 0 returns 0"""
    L = _lib.load()
    pk = peer_keys(api, 5, 0x50)
    ctx = api.curve25519_dh_Peer_Init(pk)
    n = 300
    idx = indices(5, n, 0x51, "random")
    idx[123] = 5
    sk = synth.random_bytes((n, 32), 0x0f50)
    sk0 = sk.copy()
    out = np.full((n, 32), 7, np.uint8)
    vp = C.c_void_p

    def call(shared, ctxs, n_ctx, index, s, m):
        return L.curve25519_dh_CreateSharedKey_indexed_batch(shared, ctxs, n_ctx, index, s, m)

    args = (vp(out.ctypes.data), vp(ctx.ctypes.data), 5, vp(idx.ctypes.data), vp(sk.ctypes.data), n)
    assert call(*args) != 0
    assert (out == 7).all() and np.array_equal(sk, sk0)
    with pytest.raises(_lib.EngineError):
        api.curve25519_dh_CreateSharedKey_indexed(ctx, idx, sk)
    idx[123] = 4
    assert call(args[0], args[1], 0, args[3], args[4], n) != 0
    assert call(None, args[1], 5, args[3], args[4], n) != 0
    assert call(args[0], None, 5, args[3], args[4], n) != 0
    assert call(args[0], args[1], 5, None, args[4], n) != 0
    assert call(args[0], args[1], 5, args[3], None, n) != 0
    assert call(args[0], args[1], 5, args[3], args[4], 0) == 0
    assert L.curve25519_dh_CreateSharedKey_indexed_dev(None, args[1], 5, args[3], args[4], n, None) != 0
    assert (out == 7).all() and np.array_equal(sk, sk0)
    assert L.curve25519_dh_Peer_Init_batch(None, vp(pk.ctypes.data), 5) != 0
    assert L.curve25519_dh_Peer_Init_batch(vp(ctx.ctypes.data), vp(pk.ctypes.data), 0) == 0
    got, got_sk = api.curve25519_dh_CreateSharedKey_indexed(ctx, idx, sk)
    exp, exp_sk = api.curve25519_dh_CreateSharedKey(pk[idx], sk)
    assert np.array_equal(got, exp) and np.array_equal(got_sk, exp_sk)


def test_batch_of_several_pieces_equals_dev(api):
    """the host-pointer form over several pipeline pieces equals the device form"""
    k, n = 300, 3 * (1 << 16) + 5
    pk = peer_keys(api, k, 0x60)
    ctx = api.curve25519_dh_Peer_Init(pk)
    idx = indices(k, n, 0x61, "random")
    sk = synth.random_bytes((n, 32), 0x0f60)
    got, got_sk = api.curve25519_dh_CreateSharedKey_indexed(ctx, idx, sk)
    exp, exp_sk = indexed_dev(api, to_dev(ctx), idx, sk)
    assert np.array_equal(got, exp) and np.array_equal(got_sk, exp_sk)


def test_four_threads(api):
    """four host threads at once, each with its own context set (each thread uploads into a buffer of its own)"""
    sets = [peer_keys(api, 9 + 11 * t, 0x70 + t) for t in range(4)]
    ctxs = [api.curve25519_dh_Peer_Init(pk) for pk in sets]
    jobs = [(indices(len(pk), 40_000 + 999 * t, 0x74 + t, "random"), synth.random_bytes((40_000 + 999 * t, 32), 0x0f70 + t))
            for t, pk in enumerate(sets)]
    refs = [api.curve25519_dh_CreateSharedKey(sets[t][jobs[t][0]], jobs[t][1]) for t in range(4)]
    results, errors = [[] for _ in range(4)], []

    def work(t):
        try:
            for _ in range(3):
                results[t].append(api.curve25519_dh_CreateSharedKey_indexed(ctxs[t], *jobs[t]))
            _lib.load().c25519_amd_thread_release()
        except Exception as e:                      # noqa: BLE001 (reported below)
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for t in range(4):
        assert len(results[t]) == 3
        for out, sk in results[t]:
            assert np.array_equal(out, refs[t][0]) and np.array_equal(sk, refs[t][1])


def test_kept_combs_survive(api):
    """a kept one-peer comb and a kept one-key verification comb are still walked after indexed calls on the same thread"""
    L = _lib.load()
    L.c25519_amd_thread_release()
    W = 3 << 15
    esk = synth.random_bytes((1, 32), 0x0f80)
    pub, priv = api.ed25519_CreateKeyPair(esk)
    vctx = api.ed25519_Verify_Init(pub)[0]
    msg = synth.random_bytes((1 << 16, 32), 0x0f81)
    sig = api.ed25519_SignMessage(np.repeat(priv, 1 << 16, axis=0), msg)
    assert api.ed25519_Verify_Check(vctx, sig, msg).all()
    assert L.c25519_amd_verify_check_last_wide() == 1
    peer, _ = api.curve25519_dh_CalculatePublicKey(synth.random_bytes((1, 32), 0x0f82))
    sk = synth.random_bytes((W, 32), 0x0f83)
    api.curve25519_dh_CreateSharedKey_one_peer(peer, sk)
    assert L.c25519_amd_x25519_one_peer_last_wide() == 1
    pk = peer_keys(api, 50, 0x84)
    ctx = api.curve25519_dh_Peer_Init(pk)
    for n in (1000, MIN + 1, 1 << 17):
        idx = indices(50, n, 0x85 + n, "random")
        s = synth.random_bytes((n, 32), 0x0f85 + n)
        got, _ = api.curve25519_dh_CreateSharedKey_indexed(ctx, idx, s)
        assert np.array_equal(got, api.curve25519_dh_CreateSharedKey(pk[idx], s)[0])
    got, _ = api.curve25519_dh_CreateSharedKey_one_peer(peer, sk[:4097])
    assert L.c25519_amd_x25519_one_peer_last_wide() == 1
    assert np.array_equal(got, api.curve25519_dh_CreateSharedKey(np.repeat(peer, 4097, axis=0), sk[:4097])[0])
    assert api.ed25519_Verify_Check(vctx, sig[:4096], msg[:4096]).all()
    assert L.c25519_amd_verify_check_last_wide() == 1
    L.c25519_amd_thread_release()
