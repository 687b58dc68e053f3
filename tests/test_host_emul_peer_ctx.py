"""CPU tests of X25519 against many peer contexts (curve25519_amd/csrc/x25519_peer_ctx.cuh: what curve25519_dh_Peer_Init_* and
curve25519_dh_CreateSharedKey_indexed_* run on the device).  The device source is compiled by g++ against the C model of the gfx950
primitives (tests/host_emul/peer_ctx.cpp, tests/host_emul/build.py's build_lib).  The context bytes are judged against the Python
big-integer model of the layout (tests/peer_ctx_model.py), the shared keys against the big-integer ladder of tests/one_peer_cases.py
and the reference's own curve25519_dh_CreateSharedKey where it is built.  Every peer class: KAT keys, small order, twist, u = -1,
bit 255 set, public keys of random secrets and random byte strings (some on the curve with a torsion component)."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import one_peer_cases as cases
import peer_ctx_model as model

vp, sz = C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_peer_init": ([vp, vp, sz], None), "emul_peer_indexed": ([vp, vp, sz, vp, vp, sz], C.c_long),
                    "emul_peer_gather": ([vp, vp, sz, vp, sz], None)},
                   "peer_ctx.cpp", "libc25519_emul_peer_ctx.so")
    yield lib
    assert_no_mad_overflow(lib)


def peer_init(lib, pks):
    pk = np.ascontiguousarray(np.array([np.frombuffer(bytes(p), np.uint8) for p in pks]).reshape(-1, 32))
    ctx = np.zeros((len(pk), model.CTX_SIZE), np.uint8)
    lib.emul_peer_init(ctx.ctypes.data, pk.ctypes.data, len(pk))
    return ctx


def indexed(lib, ctxs, idx, sk):
    ctxs = np.ascontiguousarray(ctxs, dtype=np.uint8)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    sk = np.ascontiguousarray(sk, dtype=np.uint8).copy()
    out = np.full_like(sk, 0xA5)
    laddered = lib.emul_peer_indexed(out.ctypes.data, ctxs.ctypes.data, len(ctxs), idx.ctypes.data, sk.ctypes.data, len(sk))
    return out, sk, laddered


def expect(pks, idx, sk, n_ctx):
    out, clamped = [], []
    for i, r in zip(idx, sk):
        k = cases.clamp(int.from_bytes(bytes(r), "little"))
        clamped.append(np.frombuffer(k.to_bytes(32, "little"), np.uint8))
        pk = pks[i] if i < n_ctx else bytes(32)
        out.append(np.frombuffer(cases.ladder(int.from_bytes(pk, "little"), k).to_bytes(32, "little"), np.uint8))
    return np.array(out), np.array(clamped)


def secrets(n, seed):
    """random secrets, plus all-ones and all-zero ones (k >> 3 = 2^251: nearly every column selects row 0) and a few with zero
    columns spread over the scalar"""
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sk[0] = 0xFF
    sk[1] = 0
    if n > 4:
        sk[2, ::2] = 0
        sk[3, 8:24] = 0
    return sk


def all_peers():
    return cases.fixed_peers() + cases.random_peers(24, 0x0f01)


def test_context_bytes_match_the_model(lib):
    """every class: the context equals the big-integer model byte for byte (key, eligibility, zero pad, 16 affine rows or zeros)"""
    peers = all_peers()
    ctx = peer_init(lib, [pk for _, pk in peers])
    for (name, pk), got in zip(peers, ctx):
        exp = np.frombuffer(model.context(pk), np.uint8)
        assert np.array_equal(got, exp), name
        assert int.from_bytes(got[32:36].tobytes(), "little") == int(cases.eligible(int.from_bytes(pk, "little"))), name


def test_small_order_contexts_are_neutral(lib):
    """Q = 8P is the neutral element: every row is (1, 1, 0), eligibility 1"""
    ctx = peer_init(lib, [cases.to_bytes(u) for u in cases.SMALL_ORDER])
    neutral = (1).to_bytes(32, "little") * 2 + bytes(32)
    for c in ctx:
        assert c[32] == 1
        assert all(c[64 + 96 * r: 160 + 96 * r].tobytes() == neutral for r in range(16))


def test_ineligible_contexts_are_zero(lib):
    """twist keys and u = -1: eligibility 0 and 1536 zero bytes of rows"""
    ctx = peer_init(lib, [cases.to_bytes(u) for u in (*cases.TWIST, *cases.MINUS_ONE)])
    assert not ctx[:, 32:].any()


def test_walk_equals_the_ladder_for_every_class(lib):
    """one call over the contexts of every class, each secret against a random context: bytes and clamped secrets equal the ladder's
    for the stored key; the elements of ineligible contexts (and only they) take the ladder"""
    peers = all_peers()
    pks = [pk for _, pk in peers]
    ctx = peer_init(lib, pks)
    rng = np.random.default_rng(0x0f10)
    n = 4 * len(pks)
    idx = np.concatenate([np.arange(len(pks)), rng.integers(0, len(pks), n - len(pks))]).astype(np.uint32)
    sk = secrets(n, 0x0f11)
    got, got_sk, laddered = indexed(lib, ctx, idx, sk)
    exp, exp_sk = expect(pks, idx, sk, len(pks))
    for i in range(n):
        assert np.array_equal(got[i], exp[i]), (peers[idx[i]][0], i)
    assert np.array_equal(got_sk, exp_sk)
    ineligible = [not cases.eligible(int.from_bytes(pk, "little")) for pk in pks]
    assert laddered == sum(ineligible[i] for i in idx)


def test_small_order_gives_zero(lib):
    ctx = peer_init(lib, [cases.to_bytes(u) for u in cases.SMALL_ORDER])
    idx = np.arange(len(ctx), dtype=np.uint32).repeat(3)
    got, _, laddered = indexed(lib, ctx, idx, secrets(len(idx), 0x0f20))
    assert laddered == 0 and not got.any()


def test_out_of_range_indices_give_zero(lib):
    """indices n_ctx, n_ctx + 1 and 2^32 - 1: 32 zero bytes, secrets still clamped, neither walk nor ladder; the gather gives key 0"""
    pks = [pk for _, pk in cases.random_peers(3, 0x0f30)]
    ctx = peer_init(lib, pks)
    idx = np.array([0, len(pks), 1, len(pks) + 1, 0xFFFFFFFF, 2, 0xFFFFFFFE], np.uint32)
    sk = secrets(len(idx), 0x0f31)
    got, got_sk, laddered = indexed(lib, ctx, idx, sk)
    exp, exp_sk = expect(pks, idx, sk, len(pks))
    assert np.array_equal(got, exp) and np.array_equal(got_sk, exp_sk)
    assert not got[[1, 3, 4, 6]].any() and laddered == 0
    keys = np.full((len(idx), 32), 0xA5, np.uint8)
    lib.emul_peer_gather(keys.ctypes.data, np.ascontiguousarray(ctx).ctypes.data, len(ctx), idx.ctypes.data, len(idx))
    for i, k in enumerate(idx):
        assert keys[i].tobytes() == (pks[k] if k < len(pks) else bytes(32))


def test_deterministic(lib):
    """the same key always gives the same bytes"""
    pks = [pk for _, pk in cases.random_peers(4, 0x0f40)]
    assert np.array_equal(peer_init(lib, pks), peer_init(lib, pks[::-1])[::-1])


def test_reference_agrees(lib, reference):
    """the reference's own curve25519_dh_CreateSharedKey on the gathered keys (where oracle/_ref is built)"""
    peers = cases.fixed_peers() + cases.random_peers(8, 0x0f50)
    pks = [pk for _, pk in peers]
    ctx = peer_init(lib, pks)
    idx = np.random.default_rng(0x0f51).integers(0, len(pks), 6 * len(pks)).astype(np.uint32)
    sk = secrets(len(idx), 0x0f52)
    got, got_sk, _ = indexed(lib, ctx, idx, sk)
    ref, ref_sk = reference.x25519_shared(np.array([np.frombuffer(pks[i], np.uint8) for i in idx]), sk)
    assert np.array_equal(got, ref) and np.array_equal(got_sk, ref_sk)
