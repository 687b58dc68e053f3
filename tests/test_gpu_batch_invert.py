"""GPU suite (MI355X): the shared inversion (csrc/batch_invert_lane.inc: k_batch_invert, the last kernel of every large batch; the
inverting wave of k_x25519_fused) at every group size it is instantiated for and with zeros on every slot of its map
(tests/invert_cases.py).  The self-test hook c25519_amd_batch_invert_selftest_dev is checked against Python big integers; every
call site of the inversion -- X25519 and its public keys, key pairs and signatures (blinded or not, both combs), reference-order
verification, verify_point, one-key Verify_Check on both outcomes, one-peer X25519 on the ladder and on the comb -- is checked
against the oracle with the group size forced by INV_K, and at the sizes where the default takes 12 and 14."""
import ctypes as C
import os

import numpy as np
import pytest

import invert_cases as cases
import one_peer_cases as peers
from curve25519_amd import _lib, synth

pytestmark = pytest.mark.gpu

THREADS = min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS") or 0) or 1 << 30)
N = 3001                                   # a few thousand ragged elements: m = ceil(N / K) is no multiple of a quad at any K


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def hook(limbs, n, k):
    import torch
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(np.ascontiguousarray(limbs).view(np.int32)).to(dev)
    d_out = torch.full((max(n, 1), 8), -0x5A5A5A5B, dtype=torch.int32, device=dev)   # (an element never written cannot pass as 0)
    _lib.check(_lib.load().c25519_amd_batch_invert_selftest_dev(C.c_void_p(d_out.data_ptr()), C.c_void_p(d_in.data_ptr()), n, k, None),
               "c25519_amd_batch_invert_selftest_dev")
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)[:n]


def low_order_rows(slots, seed):
    """element index -> a small-order peer, on the zero patterns of the slot map"""
    zeros = sorted(cases.all_zeros(cases.zero_patterns(slots, seed)))
    return {e: peers.to_bytes(peers.SMALL_ORDER[i % len(peers.SMALL_ORDER)]) for i, e in enumerate(zeros)}


def x25519_inputs(n, rows, seed):
    pk = synth.random_bytes((n, 32), seed)
    sk = synth.random_bytes((n, 32), seed + 1)
    for e, b in rows.items():
        pk[e] = np.frombuffer(b, np.uint8)
    return pk, sk


def on_device(fn, *arrays, out_widths=()):
    """one *_dev call over the whole batch (the host forms cut a batch of 2^17 rows and more into pieces, each with its own slot
    map): the arrays uploaded, outputs of the given widths, everything copied back"""
    import torch
    dev = torch.device("cuda", 0)
    n = arrays[0].shape[0]
    d_in = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    d_out = [torch.empty((n, w), dtype=torch.uint8, device=dev) for w in out_widths]
    fn(*d_out, *d_in)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in d_out + d_in]


def check_x25519(api, oracle, pk, sk, rows, what):
    got, _, clamped = on_device(api.curve25519_dh_CreateSharedKey_dev, pk, sk, out_widths=(32,))
    want, want_sk = oracle.x25519_shared(pk, sk, threads=THREADS)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first {bad[:8].tolist()}"
    assert np.array_equal(clamped, want_sk)
    z = sorted(rows)
    assert len(z) and not got[z].any(), f"{what}: a low-order peer did not give zero bytes"
    assert got[np.setdiff1d(np.arange(len(pk)), z)].any(axis=1).all()


def test_hook_against_big_integers(api):
    """every requested group size (rounding 3 -> 2, 13 -> 12, 15 -> 14; 0 = the built-in choice) at ragged sizes from 1 element to
    a few waves of quads, zeros on every slot, a whole lane, a whole quad, the last slot only, the last live lane beside partners
    past the end, and a sprinkle -- as limbs of 0, of p and inflated to the bound -- between edge vectors of the stored class"""
    for k in cases.HOOK_K:
        K = cases.group(k) if k > 0 else 1                   # (these sizes are far below 2^16: the built-in choice is 1)
        for n in cases.hook_sizes(K) + [cases.ragged_n(64 * 4 * 3 + 2, K, 1)]:
            pats = cases.zero_patterns(cases.batch_slots(n, K), seed=n)
            limbs, vals = cases.make_inputs(n, cases.all_zeros(pats), seed=n + k)
            got = hook(limbs, n, k)
            bad, count = cases.mismatches(got, cases.expected(vals), vals, pats)
            assert count == 0, f"k={k} n={n}: {count} wrong, {bad}"
    import torch
    buf = torch.zeros((64, 8), dtype=torch.int32, device=torch.device("cuda", 0))
    p = C.c_void_p(buf.data_ptr())
    assert _lib.load().c25519_amd_batch_invert_selftest_dev(p, p, 1, 17, None) != 0      # no instantiated size above 16


def test_hook_without_zeros_and_all_zero(api):
    for K in cases.INSTANTIATED:
        n = cases.ragged_n(131, K, 1)
        limbs, vals = cases.make_inputs(n, set(), seed=K)
        assert np.array_equal(hook(limbs, n, K), cases.expected(vals)), K
        limbs, vals = cases.make_inputs(n, set(range(n)), seed=K)
        assert not hook(limbs, n, K).any(), K


BATCH_PATHS = (("XF_SPLIT", 1), ("COOP_MAX", 0), ("QUAD_MAX", 0), ("LADDER2_MAX", 0))   # every call below ends in k_batch_invert


class knobs:
    def __init__(self, *pairs):
        self.t = [_lib.tunable(k, v) for k, v in pairs]

    def __enter__(self):
        for t in self.t:
            t.__enter__()

    def __exit__(self, *a):
        for t in reversed(self.t):
            t.__exit__(*a)


@pytest.mark.parametrize("K", cases.INSTANTIATED)
def test_x25519_call_sites_at_every_group_size(api, oracle, K):
    """k_batch_invert<FinishX25519, K>: shared keys with low-order peers (zero Z) on the slot map, CalculatePublicKey on the ladder
    and on the comb (_fast); one-peer X25519 with a twist peer (the ladder) and with a low-order one (every Z zero)"""
    with knobs(*BATCH_PATHS, ("INV_K", K)):
        rows = low_order_rows(cases.batch_slots(N, K), seed=K)
        pk, sk = x25519_inputs(N, rows, 0x1B00 + K)
        check_x25519(api, oracle, pk, sk, rows, f"K={K}")
        for fast in (False, True):
            got, c1 = api.curve25519_dh_CalculatePublicKey(sk, fast=fast)
            want, c2 = oracle.x25519_public(sk, fast=fast, threads=THREADS)
            assert np.array_equal(got, want) and np.array_equal(c1, c2), (K, fast)
        for u, zero in ((peers.TWIST[K % len(peers.TWIST)], False), (peers.SMALL_ORDER[K % len(peers.SMALL_ORDER)], True)):
            pb = np.frombuffer(peers.to_bytes(u), np.uint8).reshape(1, 32)
            got, clamped = api.curve25519_dh_CreateSharedKey_one_peer(pb, sk)
            want, want_sk = oracle.x25519_shared(np.repeat(pb, N, axis=0), sk, threads=THREADS)
            assert np.array_equal(got, want) and np.array_equal(clamped, want_sk), (K, u)
            assert _lib.load().c25519_amd_x25519_one_peer_last_wide() == 0
            assert (not got.any()) if zero else got.any(axis=1).all()


@pytest.mark.parametrize("K", cases.INSTANTIATED)
def test_one_peer_comb_on_quads_at_every_group_size(api, oracle, K):
    """k_batch_invert<FinishX25519IfWide, K>: a one-peer call on quads whose comb decides (built at once: ONE_PEER_WIDE = 1)"""
    n = 4001
    u = next(u for u in range(9 + 7 * K, 10**6) if peers.eligible(u))
    pb = np.frombuffer(peers.to_bytes(u), np.uint8).reshape(1, 32)
    sk = synth.random_bytes((n, 32), 0x1C00 + K)
    with knobs(("COOP_MAX", 0), ("QUAD_MIN", 0), ("QUAD_MAX", 1 << 15), ("ONE_PEER_WIDE", 1), ("INV_K", K)):
        got, clamped = api.curve25519_dh_CreateSharedKey_one_peer(pb, sk)
        assert _lib.load().c25519_amd_x25519_one_peer_last_wide() == 1
    want, want_sk = oracle.x25519_shared(np.repeat(pb, n, axis=0), sk, threads=THREADS)
    assert np.array_equal(got, want) and np.array_equal(clamped, want_sk), K


@pytest.fixture(scope="module")
def ed(oracle):
    esk = synth.random_bytes((N, 32), 0x1D01)
    msg = synth.random_bytes((N, 29), 0x1D02)
    pub, priv = oracle.ed25519_keypair(esk, threads=THREADS)
    sig = oracle.ed25519_sign(priv, msg, threads=THREADS)
    bad = sig.copy()
    bad[::5, 7] ^= 0x10                                       # R
    bad[1::5, 40] ^= 0x01                                     # S
    bmsg = msg.copy()
    bmsg[2::5, 3] ^= 0x80
    pk_bad = pub.copy()
    pk_bad[3::11, 0] ^= 0x04
    ctx = np.zeros(192, np.uint8)
    seed = np.frombuffer(b"batch inversion", np.uint8).copy()
    assert _lib.load().ed25519_Blinding_Init(ctx.ctypes.data, seed.ctypes.data, len(seed)) == ctx.ctypes.data
    return dict(esk=esk, msg=msg, pub=pub, priv=priv, sig=sig, bad=bad, bmsg=bmsg, pk_bad=pk_bad, blind=ctx,
                verdict=oracle.ed25519_verify(bad, pk_bad, bmsg, threads=THREADS))


@pytest.mark.parametrize("K", cases.INSTANTIATED)
def test_fixed_base_call_sites_at_every_group_size(api, ed, K):
    """k_batch_invert<FinishPack, K>: key pairs and signatures, blinded or not, on both combs"""
    L = _lib.load()
    for comb in (0, 1):
        with knobs(*BATCH_PATHS, ("BASE_COMB", comb), ("INV_K", K)):
            pub, priv = api.ed25519_CreateKeyPair(ed["esk"])
            assert np.array_equal(pub, ed["pub"]) and np.array_equal(priv, ed["priv"]), (K, comb)
            assert np.array_equal(api.ed25519_SignMessage(ed["priv"], ed["msg"]), ed["sig"]), (K, comb)
            bpub, bpriv, bsig = np.empty((N, 32), np.uint8), np.empty((N, 64), np.uint8), np.empty((N, 64), np.uint8)
            _lib.check(L.ed25519_CreateKeyPair_blinded_batch(bpub.ctypes.data, bpriv.ctypes.data, ed["blind"].ctypes.data,
                                                             ed["esk"].ctypes.data, N), "keypair blinded")
            _lib.check(L.ed25519_SignMessage_blinded_batch(bsig.ctypes.data, ed["priv"].ctypes.data, ed["blind"].ctypes.data,
                                                           ed["msg"].ctypes.data, ed["msg"].shape[1], N), "sign blinded")
            assert np.array_equal(bpub, ed["pub"]) and np.array_equal(bpriv, ed["priv"]) and np.array_equal(bsig, ed["sig"]), (K, comb)


@pytest.mark.parametrize("K", cases.INSTANTIATED)
def test_verification_call_sites_at_every_group_size(api, oracle, ed, K):
    """k_batch_invert<FinishVerify, K> (reference-order verification with corrupted entries; one-key Verify_Check where the two wide
    combs decide and where the reference-order kernel does) and <FinishPack, K> (verify_point)"""
    import torch
    L = _lib.load()
    with knobs(*BATCH_PATHS, ("VERIFY_REFERENCE_ORDER", 1), ("INV_K", K)):
        got = api.ed25519_VerifySignature(ed["bad"], ed["pk_bad"], ed["bmsg"])
        assert np.array_equal(got, ed["verdict"]), (K, int((got != ed["verdict"]).sum()))
        assert 0 < got.sum() < N
        dev = torch.device("cuda", 0)
        d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ed["bad"], ed["pk_bad"], ed["bmsg"])]
        out = torch.empty((N, 32), dtype=torch.uint8, device=dev)
        _lib.check(L.c25519_amd_verify_point_dev(C.c_void_p(out.data_ptr()), C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()),
                                                 C.c_void_p(d[2].data_ptr()), ed["bmsg"].shape[1], N, None), "c25519_amd_verify_point_dev")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), oracle.ed25519_verify_point(ed["bad"], ed["pk_bad"], ed["bmsg"])), K
        ctx = api.ed25519_Verify_Init(ed["pub"][:1])[0]
        one = np.repeat(ed["priv"][:1], N, axis=0)
        sig = oracle.ed25519_sign(one, ed["msg"], threads=THREADS)
        sig[::3, 50] ^= 0x02
        want = oracle.ed25519_verify(sig, np.repeat(ed["pub"][:1], N, axis=0), ed["msg"], threads=THREADS)
        for wide in (1, 0):
            with _lib.tunable("ONE_KEY_WIDE", wide):
                got = api.ed25519_Verify_Check(ctx, sig, ed["msg"])
                assert L.c25519_amd_verify_check_last_wide() == wide
            assert np.array_equal(got, want), (K, wide)


@pytest.mark.parametrize("n", ((1 << 16) + 5, (1 << 17) + 3, (1 << 18) + 7))
def test_fused_kernel_zero_slots(api, oracle, n):
    """k_x25519_fused's inverting wave (one launch: XF_SPLIT = 0) at 128 / 256 / 512 lanes per workgroup (K = 2 / 4 / 8): low-order
    peers on every slot of an inverting lane, a whole quad, the last slot only, and the last, partial workgroup"""
    block = 128 if n <= 1 << 17 else 256 if n <= 1 << 18 else 512
    slots = cases.fused_slots(n, block)
    rows = low_order_rows(slots, seed=n)
    last = (n - 1) // block * block
    assert any(e >= last for e in rows)                   # the partial workgroup has its zeros
    pk, sk = x25519_inputs(n, rows, 0x1E00 + block)
    with knobs(("XF_SPLIT", 0), ("COOP_MAX", 0), ("QUAD_MAX", 0)):
        check_x25519(api, oracle, pk, sk, rows, f"fused n={n}")


def test_default_group_sizes_12_and_14(api, oracle):
    """without knobs: n = 12 * 2^16 + 5 and 14 * 2^16 + 3 take K = 12 and 14 (the two-launch X25519 with low-order peers on the
    slot map, and key pairs), every row against the oracle"""
    for K, n in ((12, 12 * (1 << 16) + 5), (14, 14 * (1 << 16) + 3)):
        assert _lib.load().c25519_amd_tunable_get(b"INV_K") < 0
        rows = low_order_rows(cases.batch_slots(n, K), seed=K)
        pk, sk = x25519_inputs(n, rows, 0x1F00 + K)
        check_x25519(api, oracle, pk, sk, rows, f"default K={K}")
        esk = synth.random_bytes((n, 32), 0x1F10 + K)
        pub, priv, _ = on_device(api.ed25519_CreateKeyPair_dev, esk, out_widths=(32, 64))
        wpub, wpriv = oracle.ed25519_keypair(esk, threads=THREADS)
        assert np.array_equal(pub, wpub) and np.array_equal(priv, wpriv), K
