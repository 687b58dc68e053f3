"""CPU tests of ed25519_Verify_Check against many contexts in one call (curve25519_amd/csrc/verify_ctx.cuh: what
ed25519_Verify_Check_indexed_* runs on the device).  The device source -- the per-lane kernel's index gather and walk over the
context's rows, and the shared inversion's lanes with the index-aware finish -- is compiled by g++ against the C model of the gfx950
primitives (tests/host_emul/indexed_check.cpp, tests/host_emul/build.py's build_lib) and judged element by element against the
oracle's orc_ed25519_verify_check on the same 2080-byte context (orc_sigv_ctx has Verify_Init's layout).  Contexts: honest ones as
orc_ed25519_verify_init writes them and in canonical form, a flipped row byte, rows >= p, garbage keys, random bytes.  Signatures:
valid, corrupted, and R = 32 zero bytes.  Indices n_ctx - 1, n_ctx and 0xffffffff: the last two must give 0, also where R is zero
(the zero point a bad index leaves behind encodes to 32 zero bytes)."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib

P = 2**255 - 19
CTX = 2080
vp, sz = C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_indexed_check": ([vp, vp, sz, vp, vp, vp, sz, vp, sz, C.c_int, C.c_int], C.c_int)},
                   "indexed_check.cpp", "libc25519_emul_indexed_check.so")
    yield lib
    assert_no_mad_overflow(lib)


@pytest.fixture(scope="module")
def orc(oracle):
    L = oracle.lib
    L.orc_ed25519_verify_init.argtypes = [vp, vp]
    L.orc_ed25519_verify_init.restype = None
    L.orc_ed25519_verify_check.argtypes = [vp, vp, vp, sz]
    L.orc_ed25519_verify_check.restype = C.c_int
    return oracle


def verify_init(orc, pk):
    ctx = np.zeros(CTX, np.uint8)
    pk = np.ascontiguousarray(pk, np.uint8)
    orc.lib.orc_ed25519_verify_init(ctx.ctypes.data, pk.ctypes.data)
    return ctx


def fields(ctx):
    return [int.from_bytes(ctx[32 + 32 * j: 64 + 32 * j].tobytes(), "little") for j in range(64)]


def with_fields(ctx, vals):
    out = ctx.copy()
    for j, v in enumerate(vals):
        out[32 + 32 * j: 64 + 32 * j] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    return out


def context_set(orc, seed, keys):
    """(contexts uint8[n_ctx, 2080], class names, priv of the honest ones or None)"""
    rng = np.random.default_rng(seed)
    pub, priv = orc.ed25519_keypair(rng.integers(0, 256, (keys, 32), dtype=np.uint8))
    ctxs, names, privs = [], [], []

    def add(name, ctx, pv=None):
        ctxs.append(ctx); names.append(name); privs.append(pv)

    for i in range(keys):
        honest = verify_init(orc, pub[i])
        add("orc_init", honest, priv[i])
        add("canonical", with_fields(honest, [v % P for v in fields(honest)]), priv[i])
        flipped = honest.copy()
        flipped[32 + rng.integers(0, 2048)] ^= 1 << int(rng.integers(0, 8))
        add("row_byte_flipped", flipped, priv[i])
        over = [v % P for v in fields(honest)]
        over = [v + P if rng.random() < 0.5 else v for v in over]           # rows >= p (v + p < 2^256 for every v < p)
        add("rows_over_p", with_fields(honest, over), priv[i])
    for _ in range(max(2, keys // 2)):
        add("garbage_key", verify_init(orc, rng.integers(0, 256, 32, dtype=np.uint8)))
        add("random_bytes", rng.integers(0, 256, CTX, dtype=np.uint8))
    return np.stack(ctxs), names, privs


def pairs(orc, ctxs, privs, idx, seed, mlen=24):
    """signatures for ctx_index `idx` (into the set; indices past it sign with context 0's key): valid, corrupted (a bit of the
    signature or of the message), R = 32 zero bytes"""
    rng = np.random.default_rng(seed)
    n = len(idx)
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    sig = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    for i, k in enumerate(idx):
        pv = privs[k] if k < len(privs) else privs[0]
        if pv is not None:
            sig[i] = orc.ed25519_sign(pv.reshape(1, 64), msg[i].reshape(1, mlen))[0]
        kind = i % 5
        if kind == 2:
            sig[i, rng.integers(0, 64)] ^= 1 << int(rng.integers(0, 8))
        elif kind == 3 and mlen:
            msg[i, rng.integers(0, mlen)] ^= 1 << int(rng.integers(0, 8))
        elif kind == 4:
            sig[i, :32] = 0
    return sig, msg


def expect(orc, ctxs, idx, sig, msg):
    out = np.zeros(len(idx), np.int32)
    for i, k in enumerate(idx):
        if k < len(ctxs):
            c = np.ascontiguousarray(ctxs[k])
            m = np.ascontiguousarray(msg[i])
            out[i] = orc.lib.orc_ed25519_verify_check(c.ctypes.data, np.ascontiguousarray(sig[i]).ctypes.data, m.ctypes.data, m.size)
    return out


def run(lib, ctxs, idx, sig, msg=None, offsets=None, flat=None, repack=0, k=4):
    idx = np.ascontiguousarray(idx, np.uint32)
    ctxs = np.ascontiguousarray(ctxs, np.uint8)
    sig = np.ascontiguousarray(sig, np.uint8)
    n = len(idx)
    out = np.full(n, -1, np.int32)
    if offsets is not None:
        lib.emul_indexed_check(out.ctypes.data, ctxs.ctypes.data, ctxs.shape[0], idx.ctypes.data, sig.ctypes.data, flat.ctypes.data, 0,
                               offsets.ctypes.data, n, repack, k)
    else:
        msg = np.ascontiguousarray(msg, np.uint8)
        lib.emul_indexed_check(out.ctypes.data, ctxs.ctypes.data, ctxs.shape[0], idx.ctypes.data, sig.ctypes.data, msg.ctypes.data,
                               msg.shape[1], None, n, repack, k)
    return out


def test_every_context_class_against_the_oracle(lib, orc):
    """honest, canonical, flipped, rows >= p, garbage keys, random bytes; valid / corrupted / R = 0 signatures, indices in any
    order: each verdict is orc_ed25519_verify_check's on that element's context"""
    ctxs, names, privs = context_set(orc, 0x1d00, 4)
    rng = np.random.default_rng(0x1d01)
    idx = np.concatenate([np.repeat(np.arange(len(ctxs)), 5), rng.integers(0, len(ctxs), 40)]).astype(np.uint32)
    rng.shuffle(idx)
    sig, msg = pairs(orc, ctxs, privs, idx, 0x1d02)
    exp = expect(orc, ctxs, idx, sig, msg)
    got = run(lib, ctxs, idx, sig, msg)
    bad = [(i, names[idx[i]], int(got[i]), int(exp[i])) for i in np.nonzero(got != exp)[0]]
    assert not bad, bad[:10]
    ones = {names[k] for k, v in zip(idx, exp) if v}
    assert {"orc_init", "canonical", "rows_over_p"} <= ones, ones          # the honest forms do accept valid signatures


def test_indices_at_and_past_the_end(lib, orc):
    """n_ctx - 1 is a context like any other; n_ctx and 0xffffffff give 0 -- with a valid signature of context 0's key, and
    with R = 32 zero bytes, which the zero point of a bad index would otherwise match"""
    ctxs, names, privs = context_set(orc, 0x1d10, 2)
    n_ctx = len(ctxs)
    last_honest = max(i for i, p in enumerate(privs) if p is not None)
    ctxs = np.concatenate([ctxs, ctxs[last_honest:last_honest + 1]])     # the last context is an honest one
    privs = privs + [privs[last_honest]]
    n_ctx += 1
    idx = np.array([n_ctx - 1, n_ctx, 0xFFFFFFFF, 0, n_ctx, 0xFFFFFFFF, n_ctx - 1, 0x80000000] * 4, np.uint64)
    sig, msg = pairs(orc, ctxs, privs, [int(min(k, n_ctx)) for k in idx], 0x1d11)
    for i in range(len(idx)):
        if i % 8 in (4, 5):
            sig[i, :32] = 0                                                  # R = 0 behind a bad index
    idx = idx.astype(np.uint32)
    exp = expect(orc, ctxs, idx, sig, msg)
    for repack in (0, 1):
        got = run(lib, ctxs, idx, sig, msg, repack=repack)
        assert np.array_equal(got, exp), (repack, got, exp)
        assert not got[idx >= n_ctx].any()
    assert exp[(idx == n_ctx - 1)].any()                                    # the in-range neighbour does verify


def test_zero_point_with_zero_r_is_not_accepted_for_a_bad_index(lib, orc):
    """the trap of the bad-index finish: the lane leaves T = 0, the inversion maps Z = 0 to 0, enc(T) = 32 zero bytes = R"""
    ctxs, _, _ = context_set(orc, 0x1d20, 1)
    sig = np.zeros((64, 64), np.uint8)
    msg = np.zeros((64, 8), np.uint8)
    idx = np.full(64, len(ctxs), np.uint32)
    assert not run(lib, ctxs, idx, sig, msg).any()


def test_repacked_rows_and_group_sizes_agree(lib, orc):
    """the aligned copy of the rows (C25519_INDEXED_REPACK) and every inversion group size give the same verdicts"""
    ctxs, _, privs = context_set(orc, 0x1d30, 3)
    rng = np.random.default_rng(0x1d31)
    idx = rng.integers(0, len(ctxs) + 2, 70).astype(np.uint32)
    sig, msg = pairs(orc, ctxs, privs, [int(min(k, len(ctxs) - 1)) for k in idx], 0x1d32)
    exp = expect(orc, ctxs, idx, sig, msg)
    for repack, k in ((0, 1), (1, 1), (0, 16), (1, 12), (0, 2)):
        assert np.array_equal(run(lib, ctxs, idx, sig, msg, repack=repack, k=k), exp), (repack, k)


def test_ragged_messages(lib, orc):
    """per-element message lengths 0..150 through the ragged message form"""
    ctxs, _, privs = context_set(orc, 0x1d40, 2)
    rng = np.random.default_rng(0x1d41)
    n = 40
    idx = rng.integers(0, len(ctxs), n).astype(np.uint32)
    msgs = [rng.integers(0, 256, int(rng.integers(0, 151)), dtype=np.uint8) for _ in range(n)]
    msgs[0] = msgs[0][:0]
    sig = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    exp = np.zeros(n, np.int32)
    for i, k in enumerate(idx):
        if privs[k] is not None and i % 3:
            m = msgs[i].reshape(1, -1)
            sig[i] = orc.ed25519_sign(privs[k].reshape(1, 64), m)[0] if m.size else orc.ed25519_sign(privs[k].reshape(1, 64),
                                                                                                     np.zeros((1, 0), np.uint8))[0]
        m = np.ascontiguousarray(msgs[i])
        exp[i] = orc.lib.orc_ed25519_verify_check(np.ascontiguousarray(ctxs[k]).ctypes.data, np.ascontiguousarray(sig[i]).ctypes.data,
                                                  m.ctypes.data, m.size)
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum([len(m) for m in msgs], out=offsets[1:])
    flat = np.concatenate(msgs + [np.zeros(1, np.uint8)])
    got = run(lib, ctxs, idx, sig, offsets=offsets, flat=flat)
    assert np.array_equal(got, exp)
    assert exp.any()
