"""GPU suite (MI355X): ed25519_Sign_Init_* and ed25519_SignMessage_indexed_* -- n messages signed under n_ctx signer contexts in one
call.  Every signature must equal what ed25519_SignMessage_* gives with the private keys gathered (priv[ctx_index[i]]), in each of
the three forms the call size picks (one element per wave, four lanes per element, one lane per element) and with the tunables
forcing the others; the context bytes must equal the hashlib model of tests/sign_ctx_model.py."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import sign_ctx_model as model
from curve25519_amd import _lib, synth

pytestmark = pytest.mark.gpu

CTX = 128
SIZES = (1, 2, 1024, 1025, 16384, 16385, 70_000)
EDGE_LENGTHS = (0, 47, 48, 79, 80, 175, 176, 207, 208, 1000)


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


def private_keys(api, k, seed):
    _, priv = api.ed25519_CreateKeyPair(synth.random_bytes((k, 32), 0x5a0000 + seed))
    return priv


def indices(k, n, seed):
    return np.random.default_rng(seed).integers(0, k, n).astype(np.uint32)


def messages(n, size, seed):
    return synth.random_bytes((n, size), 0x5b0000 + seed) if size else np.zeros((n, 0), np.uint8)


def indexed_dev(api, d_ctx, idx, msg):
    import torch
    d_msg = to_dev(msg)
    d_sig = torch.full((len(idx), 64), 0x77, dtype=torch.uint8, device=dev())
    api.ed25519_SignMessage_indexed_dev(d_sig, d_ctx, to_dev(np.asarray(idx, np.uint32).view(np.int32).reshape(-1, 1)), d_msg)
    torch.cuda.synchronize()
    return d_sig.cpu().numpy()


def gathered_dev(api, priv, msg):
    import torch
    d_sig = torch.empty((len(priv), 64), dtype=torch.uint8, device=dev())
    api.ed25519_SignMessage_dev(d_sig, to_dev(priv), to_dev(msg))
    torch.cuda.synchronize()
    return d_sig.cpu().numpy()


def test_context_bytes(api):
    """Sign_Init (host and device forms) gives the model's bytes, also for a pk half that is another key's or not a point"""
    import torch
    priv = private_keys(api, 50, 1)
    priv[3, 32:] = priv[4, 32:]
    priv[7, 32:] = np.arange(32, dtype=np.uint8)
    ctx = api.ed25519_Sign_Init(priv)
    for i in range(len(priv)):
        assert ctx[i].tobytes() == model.sign_ctx(priv[i].tobytes()), i
    d_ctx = torch.zeros((len(priv), CTX), dtype=torch.uint8, device=dev())
    api.ed25519_Sign_Init_dev(d_ctx, to_dev(priv))
    torch.cuda.synchronize()
    assert np.array_equal(d_ctx.cpu().numpy(), ctx)


@pytest.mark.parametrize("n", SIZES)
def test_parity_with_sign_message(api, n):
    """at the dispatch edges of the three forms: the host form equals SignMessage_batch and the device form SignMessage_dev on the
    gathered keys (64 keys, 32-byte messages, random indices; a pk half of another key among them)"""
    priv = private_keys(api, 64, 2)
    priv[5, 32:] = priv[6, 32:]
    ctx = api.ed25519_Sign_Init(priv)
    idx = indices(64, n, 0x20 + n)
    msg = messages(n, 32, 0x21 + n)
    exp = api.ed25519_SignMessage(priv[idx], msg)
    assert np.array_equal(api.ed25519_SignMessage_indexed(ctx, idx, msg), exp)
    assert np.array_equal(indexed_dev(api, to_dev(ctx), idx, msg), exp)
    assert np.array_equal(gathered_dev(api, priv[idx], msg), exp)


@pytest.mark.parametrize("knob,n", [("QUAD_MAX", 1025), ("QUAD_MAX", 2048), ("QUAD_MAX", 16384), ("COOP_MAX", 1), ("COOP_MAX", 1024),
                                    ("COOP_MAX", 1025), ("BASE_COMB", 7), ("BASE_COMB", 70_000)])
def test_forced_forms(api, n, knob):
    """QUAD_MAX = 0 (no quads: per wave up to 2048, then per lane), COOP_MAX = 0 (never per wave), BASE_COMB = 0 (the LDS comb:
    per wave and per lane over it) -- restored afterwards; the bytes stay SignMessage_dev's under the default dispatch"""
    priv = private_keys(api, 33, 3)
    ctx = to_dev(api.ed25519_Sign_Init(priv))
    idx = indices(33, n, 0x30 + n)
    msg = messages(n, 32, 0x31 + n)
    exp = gathered_dev(api, priv[idx], msg)
    L = _lib.load()
    prev = L.c25519_amd_tunable_get(knob.encode())
    try:
        assert L.c25519_amd_tunable_set(knob.encode(), 0) == 0
        assert np.array_equal(indexed_dev(api, ctx, idx, msg), exp)
        assert np.array_equal(gathered_dev(api, priv[idx], msg), exp)
    finally:
        L.c25519_amd_tunable_set(knob.encode(), prev)
    assert L.c25519_amd_tunable_get(knob.encode()) == prev


@pytest.mark.parametrize("n", (10, 2000, 20_000))
def test_ragged_messages(api, n):
    """per-element lengths on both sides of each SHA-512 block edge of the two hashes, per wave / quad / lane"""
    priv = private_keys(api, 17, 4)
    ctx = api.ed25519_Sign_Init(priv)
    idx = indices(17, n, 0x40 + n)
    rng = np.random.default_rng(0x41 + n)
    msgs = [rng.integers(0, 256, EDGE_LENGTHS[i % len(EDGE_LENGTHS)] if i < 4 * len(EDGE_LENGTHS) else int(rng.integers(0, 300)),
                         dtype=np.uint8).tobytes() for i in range(n)]
    exp = api.ed25519_SignMessage_ragged(priv[idx], msgs)
    assert np.array_equal(api.ed25519_SignMessage_indexed_ragged(ctx, idx, msgs), exp)
    flat, offsets = api._ragged(msgs)
    import torch
    d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev())
    L = _lib.load()
    d_flat, d_off, d_idx = to_dev(np.concatenate([flat, np.zeros(16, np.uint8)])), to_dev(offsets), to_dev(idx.view(np.int32))
    d_ctx = to_dev(ctx)
    with api._on(d_sig) as st:
        rc = L.ed25519_SignMessage_indexed_ragged_dev(d_sig.data_ptr(), d_ctx.data_ptr(), len(ctx), d_idx.data_ptr(), d_flat.data_ptr(),
                                                      C.c_void_p(d_off.data_ptr()), n, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_sig.cpu().numpy(), exp)


def test_many_contexts(api):
    """K = 70 000 contexts (8.96 MB), every one used"""
    k, n = 70_000, 100_000
    priv = private_keys(api, k, 5)
    ctx = api.ed25519_Sign_Init(priv)
    idx = np.concatenate([np.arange(k, dtype=np.uint32), indices(k, n - k, 0x50)])
    np.random.default_rng(0x51).shuffle(idx)
    msg = messages(n, 32, 0x52)
    exp = gathered_dev(api, priv[idx], msg)
    assert np.array_equal(indexed_dev(api, to_dev(ctx), idx, msg), exp)
    assert np.array_equal(api.ed25519_SignMessage_indexed(ctx, idx, msg), exp)


def test_digest_at_2_20(api):
    """a 2^20 call over 4096 contexts: the SHA-256 of its signatures is that of SignMessage_dev on the gathered keys"""
    n = 1 << 20
    priv = private_keys(api, 4096, 6)
    ctx = to_dev(api.ed25519_Sign_Init(priv))
    idx = indices(4096, n, 0x60)
    msg = messages(n, 32, 0x61)
    got = hashlib.sha256(indexed_dev(api, ctx, idx, msg).tobytes()).hexdigest()
    exp = hashlib.sha256(gathered_dev(api, priv[idx], msg).tobytes()).hexdigest()
    assert got == exp


@pytest.mark.parametrize("n", (3, 1500, 20_000))
def test_bad_indices_on_dev(api, n):
    """the device form: an index >= n_ctx (n_ctx itself, 0xffffffff, 2^31) gives 64 zero bytes, its neighbours their signatures"""
    priv = private_keys(api, 9, 7)
    ctx = to_dev(api.ed25519_Sign_Init(priv))
    idx = indices(9, n, 0x70 + n)
    idx[:: 7] = 9
    idx[1:: 11] = 0xFFFFFFFF
    idx[2:: 13] = 0x80000000
    if n == 3:
        idx[:] = (8, 9, 0xFFFFFFFF)
    msg = messages(n, 32, 0x71 + n)
    got = indexed_dev(api, ctx, idx, msg)
    bad = idx >= 9
    assert bad.any() and not got[bad].any()
    exp = gathered_dev(api, priv[np.where(bad, 0, idx)], msg)
    assert np.array_equal(got[~bad], exp[~bad])


def test_host_refusals(api):
    """_batch: an out-of-range index refuses the call with sig untouched; n_ctx = 0 and null pointers are argument errors; n = 0
    returns 0"""
    L = _lib.load()
    priv = private_keys(api, 5, 8)
    ctx = api.ed25519_Sign_Init(priv)
    n = 300
    idx = indices(5, n, 0x80)
    idx[123] = 5
    msg = messages(n, 32, 0x81)
    sig = np.full((n, 64), 7, np.uint8)
    vp = C.c_void_p
    args = [vp(sig.ctypes.data), vp(ctx.ctypes.data), 5, vp(idx.ctypes.data), vp(msg.ctypes.data), 32, n]
    assert L.ed25519_SignMessage_indexed_batch(*args) != 0
    assert (sig == 7).all()
    with pytest.raises(_lib.EngineError):
        api.ed25519_SignMessage_indexed(ctx, idx, msg)
    offsets = np.arange(n + 1, dtype=np.uint64) * 32
    assert L.ed25519_SignMessage_indexed_ragged_batch(args[0], args[1], 5, args[3], args[4], vp(offsets.ctypes.data), n) != 0
    assert (sig == 7).all()
    idx[123] = 4
    for j, bad in ((2, 0), (0, None), (1, None), (3, None), (4, None)):
        a = list(args)
        a[j] = bad
        assert L.ed25519_SignMessage_indexed_batch(*a) != 0, j
    a = list(args)
    a[6] = 0
    assert L.ed25519_SignMessage_indexed_batch(*a) == 0
    assert L.ed25519_SignMessage_indexed_dev(None, args[1], 5, args[3], args[4], 32, n, None) != 0
    assert L.ed25519_Sign_Init_batch(None, vp(priv.ctypes.data), 5) != 0
    assert L.ed25519_Sign_Init_batch(vp(ctx.ctypes.data), vp(priv.ctypes.data), 0) == 0
    assert (sig == 7).all()
    assert L.ed25519_SignMessage_indexed_batch(*args) == 0
    assert np.array_equal(sig, api.ed25519_SignMessage(priv[idx], msg))


def test_batch_of_several_pieces_equals_dev(api):
    """the host-pointer form over several pipeline pieces equals the device form"""
    k, n = 300, 3 * (1 << 16) + 5
    priv = private_keys(api, k, 9)
    ctx = api.ed25519_Sign_Init(priv)
    idx = indices(k, n, 0x90)
    msg = messages(n, 32, 0x91)
    assert np.array_equal(api.ed25519_SignMessage_indexed(ctx, idx, msg), indexed_dev(api, to_dev(ctx), idx, msg))


def test_two_threads(api):
    """two host threads at once, each with its own key set (each thread uploads into a buffer of its own)"""
    sets = [private_keys(api, 11 + 20 * t, 0xa0 + t) for t in range(2)]
    ctxs = [api.ed25519_Sign_Init(p) for p in sets]
    jobs = [(indices(len(p), 50_000 + 777 * t, 0xa4 + t), messages(50_000 + 777 * t, 32, 0xa6 + t)) for t, p in enumerate(sets)]
    refs = [api.ed25519_SignMessage(sets[t][jobs[t][0]], jobs[t][1]) for t in range(2)]
    results, errors = [[] for _ in range(2)], []

    def work(t):
        try:
            for _ in range(3):
                results[t].append(api.ed25519_SignMessage_indexed(ctxs[t], *jobs[t]))
            _lib.load().c25519_amd_thread_release()
        except Exception as e:                      # noqa: BLE001 (reported below)
            errors.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for t in range(2):
        assert len(results[t]) == 3
        for sig in results[t]:
            assert np.array_equal(sig, refs[t])
