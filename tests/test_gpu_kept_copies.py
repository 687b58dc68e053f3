"""GPU suite (MI355X): the per-thread device copies of caller data behind the host-pointer (*_batch) calls -- three records that
are uploaded only when their bytes change (the Verify_Check context, the blinding context, the one-peer key) and three grow-only
context arrays that are uploaded on every indexed call (capi_common.hpp: KeptRecord, GrowArray).  Every case runs on one thread
and compares the *_batch form with the *_dev form on the same inputs.

What other files pin already, and is not repeated here: a record that changes between two calls of one thread is uploaded again --
test_gpu_parity.py::test_two_phase_verification checks five Verify_Init contexts in turn against the oracle, and
test_gpu_one_peer.py::test_batch_form_and_threads two peer keys in turn against the ladder.  The blinding record cannot be pinned
by bytes at all: blinded outputs do not depend on the context (test_blinding_contexts_are_real_and_output_neutral), so a stale
upload would give the same signatures; here it only passes through a thread's exit with the others."""
import threading

import numpy as np
import pytest

from curve25519_amd import _lib, synth

pytestmark = pytest.mark.gpu

N = 3000                              # elements per call: the per-lane kernels of all three calls
MANY = 4096                           # contexts of the large step: 8.5 MB / 6.5 MB / 0.5 MB of verification / peer / signer contexts


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def indices(k, seed):
    """N indices into k contexts; the first and the last context are always among them"""
    idx = np.random.default_rng(seed).integers(0, k, N).astype(np.uint32)
    idx[0], idx[-1] = 0, k - 1
    return idx


def dev_idx(idx):
    return to_dev(idx.view(np.int32).reshape(-1, 1))


def check_case(api, k, seed):
    """k verification contexts; signatures under the indexed key, every 7th corrupted, every 13th index moved to another key"""
    import torch
    pub, priv = api.ed25519_CreateKeyPair(synth.random_bytes((k, 32), 0xca0000 + seed))
    ctxs = api.ed25519_Verify_Init(pub)
    idx = indices(k, seed)
    msg = synth.random_bytes((N, 24), 0xca1000 + seed)
    sig = api.ed25519_SignMessage(priv[idx], msg)
    sig[::7, 40] ^= 4
    if k > 1:
        idx[5::13] = (idx[5::13] + 1) % k
    d_ok = torch.full((N, 1), -1, dtype=torch.int32, device=torch.device("cuda", 0))
    api.ed25519_Verify_Check_indexed_dev(d_ok, to_dev(ctxs), dev_idx(idx), to_dev(sig), to_dev(msg))
    torch.cuda.synchronize()
    exp = d_ok.cpu().numpy().reshape(-1)
    assert 0.5 < exp.mean() < 0.95
    return (lambda: api.ed25519_Verify_Check_indexed(ctxs, idx, sig, msg)), exp


def sign_case(api, k, seed):
    import torch
    _, priv = api.ed25519_CreateKeyPair(synth.random_bytes((k, 32), 0xcb0000 + seed))
    ctxs = api.ed25519_Sign_Init(priv)
    idx = indices(k, seed)
    msg = synth.random_bytes((N, 24), 0xcb1000 + seed)
    d_sig = torch.zeros((N, 64), dtype=torch.uint8, device=torch.device("cuda", 0))
    api.ed25519_SignMessage_indexed_dev(d_sig, to_dev(ctxs), dev_idx(idx), to_dev(msg))
    torch.cuda.synchronize()
    return (lambda: api.ed25519_SignMessage_indexed(ctxs, idx, msg)), d_sig.cpu().numpy()


def peer_case(api, k, seed):
    import torch
    pk, _ = api.curve25519_dh_CalculatePublicKey(synth.random_bytes((k, 32), 0xcc0000 + seed))
    ctxs = api.curve25519_dh_Peer_Init(pk)
    idx = indices(k, seed)
    sk = synth.random_bytes((N, 32), 0xcc1000 + seed)
    d_sk = to_dev(sk)
    d_out = torch.empty_like(d_sk)
    api.curve25519_dh_CreateSharedKey_indexed_dev(d_out, to_dev(ctxs), dev_idx(idx), d_sk)
    torch.cuda.synchronize()
    return (lambda: api.curve25519_dh_CreateSharedKey_indexed(ctxs, idx, sk)[0]), d_out.cpu().numpy()


CASES = {"check": check_case, "sign": sign_case, "peer": peer_case}


def run(api, call, k, seed):
    batch, exp = CASES[call](api, k, seed)
    assert np.array_equal(batch(), exp), (call, k, seed)


@pytest.mark.parametrize("call", sorted(CASES))
def test_context_array_grows_shrinks_and_grows(api, call):
    """4, then 4096, then 4 contexts (other keys each time), then 4096 again after the thread's buffers were released: the call
    reads the contexts it was given, not what an earlier call left in the buffer"""
    _lib.load().c25519_amd_thread_release()
    for step, k in enumerate((4, MANY, 4)):
        run(api, call, k, 16 * step + 1)
    _lib.load().c25519_amd_thread_release()
    run(api, call, MANY, 0x41)


@pytest.mark.parametrize("call", sorted(CASES))
def test_release_between_two_calls(api, call):
    """c25519_amd_thread_release() frees the kept array; the next call on the thread allocates and uploads again"""
    run(api, call, 37, 0x51)
    _lib.load().c25519_amd_thread_release()
    run(api, call, 37, 0x52)
    run(api, call, 37, 0x51)


def test_all_six_kept_copies_pass_through_a_thread_exit(api):
    """Short-lived threads that each make the three indexed calls (4096 contexts: 15.5 MB of kept arrays per thread), a one-peer
    call, a Verify_Check call and a blinded signing call, all with the right answers, and exit without calling
    c25519_amd_thread_release(): device memory must not grow.  Eight leaked threads would hold 124 MB; the bound is
    test_thread_resources_are_released's 16 MiB.  That bound sees the three context arrays only: a leaked record of 2080, 192 or 32
    bytes is far below it, so for the three records this test pins that a thread which used them exits without a fault and that
    later threads still get right answers, not that their bytes were freed.  (The blinded call's bytes cannot show whether its
    context was uploaded either: module docstring.)"""
    import torch
    L = _lib.load()
    indexed = [CASES[c](api, MANY, 0x61) for c in sorted(CASES)]
    # one key, one peer, one blinding context
    pub, priv = api.ed25519_CreateKeyPair(synth.random_bytes((1, 32), 0xcd01))
    vctx = api.ed25519_Verify_Init(pub)[0]
    msg = synth.random_bytes((N, 24), 0xcd02)
    sig = api.ed25519_SignMessage(np.repeat(priv, N, axis=0), msg)
    bad = sig.copy()
    bad[::5, 40] ^= 1
    peer, _ = api.curve25519_dh_CalculatePublicKey(synth.random_bytes((1, 32), 0xcd03))
    sk = synth.random_bytes((N, 32), 0xcd04)
    shared, _ = api.curve25519_dh_CreateSharedKey(np.repeat(peer, N, axis=0), sk)
    bctx = np.zeros(192, np.uint8)
    assert L.ed25519_Blinding_Init(bctx.ctypes.data, b"kept copies", 11) == bctx.ctypes.data
    privs = np.ascontiguousarray(np.repeat(priv, N, axis=0))
    errors = []

    def work():
        try:
            for j, (batch, exp) in enumerate(indexed):
                if not np.array_equal(batch(), exp):
                    errors.append(("indexed", j))
            if not np.array_equal(api.curve25519_dh_CreateSharedKey_one_peer(peer, sk)[0], shared):
                errors.append("one peer")
            if not np.array_equal(api.ed25519_Verify_Check(vctx, bad, msg) == 1, np.arange(N) % 5 != 0):
                errors.append("verify check")
            bsig = np.zeros((N, 64), np.uint8)
            _lib.check(L.ed25519_SignMessage_blinded_batch(bsig.ctypes.data, privs.ctypes.data, bctx.ctypes.data, msg.ctypes.data,
                                                           msg.shape[1], N), "sign blinded")
            if not np.array_equal(bsig, sig):
                errors.append("blinded")
        except Exception as e:                                  # noqa: BLE001
            errors.append(repr(e))

    def churn(k):
        for _ in range(k):
            th = threading.Thread(target=work)
            th.start()
            th.join()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    work()
    L.c25519_amd_thread_release()
    free_a = churn(2)                                      # the HIP runtime may keep one freed block cached: settle first
    free_b = churn(8)
    assert not errors, errors
    assert free_a - free_b < 16 << 20, (free_a, free_b)
    work()                                                  # and the main thread still works after its own release
    assert not errors, errors
