"""GPU suite (MI355X): ed25519_Verify_Check_indexed_* -- n (context index, signature, message) triples against n_ctx Verify_Init
contexts in one call.  Element i's verdict must be what ed25519_Verify_Check gives for context ctx_index[i] (one call per context
group), and for honest contexts what ed25519_VerifySignature gives for pk = pub[ctx_index[i]]; an index >= n_ctx gives 0 on the
device and refuses a host-pointer call."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

from curve25519_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def keyset(api, k, seed):
    rng = np.random.default_rng(seed)
    pub, priv = api.ed25519_CreateKeyPair(rng.integers(0, 256, (k, 32), dtype=np.uint8))
    return pub, priv, api.ed25519_Verify_Init(pub)


def mixed(api, pub, priv, n, seed, mlen=40, wrong=True):
    """n triples over the keys: valid signatures, a corrupted signature or message in every 7th / 11th, and (wrong) every 13th
    index pointing at another key than the one that signed"""
    rng = np.random.default_rng(seed)
    k = len(pub)
    idx = rng.integers(0, k, n).astype(np.uint32)
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    sig = api.ed25519_SignMessage(priv[idx], msg)
    sig[::7, 40] ^= 4
    if mlen:
        msg[3::11, 0] ^= 1
    if wrong and k > 1:
        idx[5::13] = (idx[5::13] + 1 + rng.integers(0, k - 1, len(idx[5::13]))) % k
    return idx, sig, msg


def per_group(api, ctxs, idx, sig, msg):
    """one ed25519_Verify_Check call per context group"""
    out = np.full(len(idx), -1, np.int32)
    for c in np.unique(idx):
        sel = np.nonzero(idx == c)[0]
        out[sel] = api.ed25519_Verify_Check(ctxs[c], sig[sel], msg[sel])
    return out


def test_mixed_keys_against_oracle_and_groups(api, oracle):
    """37 device-made keys, 5000 triples in random order, corrupted signatures / messages and wrong keys"""
    pub, priv, ctxs = keyset(api, 37, 0x2a00)
    idx, sig, msg = mixed(api, pub, priv, 5000, 0x2a01)
    got = api.ed25519_Verify_Check_indexed(ctxs, idx, sig, msg)
    exp = oracle.ed25519_verify(sig, pub[idx], msg).astype(np.int32)
    assert np.array_equal(got, exp)
    assert np.array_equal(got, per_group(api, ctxs, idx, sig, msg))
    assert 0.5 < got.mean() < 0.95


def test_tampered_and_garbage_contexts(api):
    """contexts not written by Verify_Init -- a flipped row byte, rows + p, a random key's table, random bytes -- in the same call
    as honest ones: every element equals its context's own Verify_Check call"""
    rng = np.random.default_rng(0x2a10)
    pub, priv, ctxs = keyset(api, 6, 0x2a11)
    P = 2**255 - 19
    bad = []
    for i in range(6):
        c = ctxs[i].copy()
        c[32 + rng.integers(0, 2048)] ^= 1 << int(rng.integers(0, 8))
        bad.append(c)
        c = ctxs[i].copy()
        for j in range(0, 64, 3):
            v = int.from_bytes(c[32 + 32 * j: 64 + 32 * j].tobytes(), "little")
            c[32 + 32 * j: 64 + 32 * j] = np.frombuffer(((v % P) + P).to_bytes(32, "little"), np.uint8)
        bad.append(c)
    bad.append(api.ed25519_Verify_Init(rng.integers(0, 256, (1, 32), dtype=np.uint8))[0])
    bad.append(rng.integers(0, 256, 2080, dtype=np.uint8))
    all_ctx = np.concatenate([ctxs, np.stack(bad)])
    idx, sig, msg = mixed(api, pub, priv, 3000, 0x2a12, wrong=False)
    idx = np.where(np.arange(3000) % 2 == 0, idx, 6 + rng.integers(0, len(bad), 3000)).astype(np.uint32)
    got = api.ed25519_Verify_Check_indexed(all_ctx, idx, sig, msg)
    assert np.array_equal(got, per_group(api, all_ctx, idx, sig, msg))
    assert got[idx < 6].mean() > 0.5


@pytest.mark.parametrize("n", [1, 2, 1024, 1025])
def test_per_wave_and_per_lane_agree(api, n):
    """n at the COOP_MAX edge, with the default (per wave up to 1024) and COOP_MAX = 0 (always per lane)"""
    L = _lib.load()
    pub, priv, ctxs = keyset(api, 9, 0x2a20)
    idx, sig, msg = mixed(api, pub, priv, n, 0x2a21 + n)
    ref = per_group(api, ctxs, idx, sig, msg)
    got = api.ed25519_Verify_Check_indexed(ctxs, idx, sig, msg)
    try:
        assert L.c25519_amd_tunable_set(b"COOP_MAX", 0) == 0
        lane = api.ed25519_Verify_Check_indexed(ctxs, idx, sig, msg)
    finally:
        L.c25519_amd_tunable_set(b"COOP_MAX", -1)
    assert np.array_equal(got, ref) and np.array_equal(lane, ref)


def test_batch_larger_than_one_piece(api):
    """2^18 + 77 triples through the host pipeline's pieces; digest against the per-group calls"""
    n = (1 << 18) + 77
    pub, priv, ctxs = keyset(api, 37, 0x2a30)
    idx, sig, msg = mixed(api, pub, priv, n, 0x2a31, mlen=32)
    got = api.ed25519_Verify_Check_indexed(ctxs, idx, sig, msg)
    ref = per_group(api, ctxs, idx, sig, msg)
    assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(ref.tobytes()).hexdigest()
    assert 0.5 < got.mean() < 0.95


def test_contexts_beyond_l2(api, oracle):
    """70 000 contexts (146 MB, beyond an XCD's L2): sampled elements against the oracle"""
    k = 70_000
    pub, priv, ctxs = keyset(api, k, 0x2a40)
    idx, sig, msg = mixed(api, pub, priv, 1 << 17, 0x2a41, mlen=16)
    got = api.ed25519_Verify_Check_indexed(ctxs, idx, sig, msg)
    s = np.random.default_rng(0x2a42).choice(len(idx), 4000, replace=False)
    exp = oracle.ed25519_verify(sig[s], pub[idx[s]], msg[s]).astype(np.int32)
    assert np.array_equal(got[s], exp)
    assert len(np.unique(idx)) > 50_000


def test_ragged_messages(api):
    """messages of 0..300 bytes against ed25519_VerifySignature_ragged with pk = pub[idx]"""
    rng = np.random.default_rng(0x2a50)
    pub, priv, ctxs = keyset(api, 23, 0x2a51)
    n = 3000
    idx = rng.integers(0, 23, n).astype(np.uint32)
    messages = [rng.integers(0, 256, int(rng.integers(0, 301)), dtype=np.uint8).tobytes() for _ in range(n)]
    sig = api.ed25519_SignMessage_ragged(priv[idx], messages)
    sig[::9, 33] ^= 1
    idx[4::17] = (idx[4::17] + 1) % 23
    got = api.ed25519_Verify_Check_indexed_ragged(ctxs, idx, sig, messages)
    exp = api.ed25519_VerifySignature_ragged(sig, pub[idx], messages)
    assert np.array_equal(got, exp)
    assert 0.5 < got.mean() < 0.95


def test_out_of_range_indices(api):
    """_dev: verdict 0 exactly where the index is >= n_ctx, correct elsewhere (per wave and per lane); _batch: one bad index is an
    error and leaves the verdicts untouched; n_ctx = 1 with every index 0 equals Verify_Check(ctx[0])"""
    import torch
    pub, priv, ctxs = keyset(api, 5, 0x2a60)
    dev = torch.device("cuda", 0)
    for n in (700, 5000):
        idx, sig, msg = mixed(api, pub, priv, n, 0x2a61 + n)
        bad = np.zeros(n, bool)
        bad[::10] = True
        idx_b = idx.copy()
        idx_b[bad] = np.where(np.arange(bad.sum()) % 2 == 0, 5, 0xFFFFFFFF)
        sig_b = sig.copy()
        sig_b[bad.nonzero()[0][::3], :32] = 0                              # R = 0 behind a bad index: still 0
        ref_b = per_group(api, ctxs, idx[~bad], sig_b[~bad], msg[~bad])
        d_v = torch.full((n, 1), -1, dtype=torch.int32, device=dev)
        api.ed25519_Verify_Check_indexed_dev(d_v, torch.from_numpy(ctxs).to(dev), torch.from_numpy(idx_b.view(np.int32).reshape(n, 1)).to(dev),
                                             torch.from_numpy(sig_b).to(dev), torch.from_numpy(msg).to(dev))
        torch.cuda.synchronize()
        v = d_v.cpu().numpy().reshape(-1)
        assert not v[bad].any()
        assert np.array_equal(v[~bad], ref_b)
    idx, sig, msg = mixed(api, pub, priv, 300, 0x2a62)
    idx[123] = 5
    out = np.full(300, 7, np.int32)
    L = _lib.load()
    rc = L.ed25519_Verify_Check_indexed_batch(C.c_void_p(out.ctypes.data), C.c_void_p(ctxs.ctypes.data), 5, C.c_void_p(idx.ctypes.data),
                                              C.c_void_p(sig.ctypes.data), C.c_void_p(msg.ctypes.data), msg.shape[1], 300)
    assert rc != 0 and (out == 7).all()
    with pytest.raises(_lib.EngineError):
        api.ed25519_Verify_Check_indexed(ctxs, idx, sig, msg)
    assert L.ed25519_Verify_Check_indexed_batch(C.c_void_p(out.ctypes.data), C.c_void_p(ctxs.ctypes.data), 0, C.c_void_p(idx.ctypes.data),
                                                C.c_void_p(sig.ctypes.data), C.c_void_p(msg.ctypes.data), msg.shape[1], 300) != 0
    assert L.ed25519_Verify_Check_indexed_batch(C.c_void_p(out.ctypes.data), C.c_void_p(ctxs.ctypes.data), 5, C.c_void_p(idx.ctypes.data),
                                                C.c_void_p(sig.ctypes.data), C.c_void_p(msg.ctypes.data), msg.shape[1], 0) == 0
    assert (out == 7).all()
    for n in (3, 2000):
        idx, sig, msg = mixed(api, pub[:1], priv[:1], n, 0x2a63 + n)
        got = api.ed25519_Verify_Check_indexed(ctxs[:1], np.zeros(n, np.uint32), sig, msg)
        assert np.array_equal(got, api.ed25519_Verify_Check(ctxs[0], sig, msg))


def test_two_threads(api):
    """two host threads at once, each with its own context set (each thread's contexts live in a buffer of its own)"""
    sets = [keyset(api, 11 + 6 * t, 0x2a70 + t) for t in range(2)]
    jobs = [mixed(api, pub, priv, 20_000, 0x2a72 + t) for t, (pub, priv, _) in enumerate(sets)]
    refs = [per_group(api, sets[t][2], *jobs[t]) for t in range(2)]
    results, errors = [[], []], []

    def work(t):
        try:
            for _ in range(4):
                results[t].append(api.ed25519_Verify_Check_indexed(sets[t][2], *jobs[t]))
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
        assert len(results[t]) == 4 and all(np.array_equal(r, refs[t]) for r in results[t])
