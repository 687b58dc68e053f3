"""CPU tests of Ed25519 signing against many signer contexts in one call (curve25519_amd/csrc/sign_ctx.cuh: what ed25519_Sign_Init_*
and ed25519_SignMessage_indexed_* run on the device).  The device source -- the context build, and all three signing forms (one lane
per element around the shared inversion, four lanes per element, one element per two-wave workgroup over the LDS comb and the wide
comb) -- is compiled by g++ against the C model of the gfx950 primitives (tests/host_emul/sign_ctx.cpp, the recipe of
tests/host_emul/build.py) and judged against the oracle's orc_ed25519_sign on the gathered private keys, and against the big-integer
model of tests/sign_ctx_model.py for contexts that no private key gives (random bytes, an unclamped a).  Message lengths sit on both
sides of each SHA-512 block edge of the two prefixed hashes (H(prefix || m): 32 + len + 17 bytes; H(enc(R) || pk || m): 64 + len +
17).  Indices n_ctx and 0xffffffff give 64 zero bytes."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import sign_ctx_model as model

CTX = 128
FORMS = [(0, 0, "lane/lds-comb"), (0, 1, "lane/wide"), (1, 1, "quad"), (2, 0, "wave/lds-comb"), (2, 1, "wave/wide")]
EDGE_LENGTHS = [0, 47, 48, 79, 80, 175, 176, 207, 208, 1000]
vp, sz = C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_sign_ctx_init": ([vp, vp, sz], None),
                    "emul_sign_indexed": ([vp, vp, sz, vp, vp, sz, vp, sz, C.c_int, C.c_int], None)},
                   "sign_ctx.cpp", "libc25519_emul_sign_ctx.so")
    yield lib
    assert_no_mad_overflow(lib)


def keys(orc, k, seed):
    rng = np.random.default_rng(seed)
    _, priv = orc.ed25519_keypair(rng.integers(0, 256, (k, 32), dtype=np.uint8))
    return priv


def init(lib, priv):
    priv = np.ascontiguousarray(priv, np.uint8)
    out = np.zeros((priv.shape[0], CTX), np.uint8)
    lib.emul_sign_ctx_init(out.ctypes.data, priv.ctypes.data, priv.shape[0])
    return out


def run(lib, ctxs, idx, form, wide, msg=None, messages=None):
    ctxs = np.ascontiguousarray(ctxs, np.uint8)
    idx = np.ascontiguousarray(idx, np.uint32)
    n = len(idx)
    sig = np.full((n, 64), 0x5A, np.uint8)
    if messages is not None:
        offsets = np.zeros(n + 1, np.uint64)
        np.cumsum([len(m) for m in messages], out=offsets[1:])
        flat = np.concatenate([np.frombuffer(bytes(m), np.uint8) for m in messages] + [np.zeros(1, np.uint8)])
        lib.emul_sign_indexed(sig.ctypes.data, ctxs.ctypes.data, ctxs.shape[0], idx.ctypes.data, flat.ctypes.data, 0,
                              offsets.ctypes.data, n, form, wide)
    else:
        msg = np.ascontiguousarray(msg, np.uint8)
        lib.emul_sign_indexed(sig.ctypes.data, ctxs.ctypes.data, ctxs.shape[0], idx.ctypes.data, msg.ctypes.data, msg.shape[1], None,
                              n, form, wide)
    return sig


def oracle_sigs(orc, priv, idx, messages):
    return np.stack([orc.ed25519_sign(priv[k].reshape(1, 64), np.frombuffer(bytes(m), np.uint8).reshape(1, -1))[0]
                     for k, m in zip(idx, messages)])


def test_init_matches_the_hashlib_model(lib, orc_keys):
    """a = clamp(H(seed)[0..31]), prefix = H(seed)[32..63], pk as given, 32 zero bytes -- also for a pk half of another key"""
    priv = orc_keys.copy()
    priv[1, 32:] = priv[0, 32:]
    ctxs = init(lib, priv)
    for i in range(len(priv)):
        assert ctxs[i].tobytes() == model.sign_ctx(priv[i].tobytes()), i


@pytest.fixture(scope="module")
def orc_keys(oracle):
    return keys(oracle, 6, 0x5c00)


@pytest.mark.parametrize("form,wide,name", FORMS, ids=[f[2] for f in FORMS])
def test_honest_contexts_equal_the_oracle(lib, oracle, orc_keys, form, wide, name):
    """contexts from Sign_Init on the oracle's private keys, indices in any order, 40-byte messages: orc_ed25519_sign's bytes"""
    rng = np.random.default_rng(0x5c10 + form * 2 + wide)
    ctxs = init(lib, orc_keys)
    n = 24 if form == 2 else 37
    idx = rng.integers(0, len(orc_keys), n).astype(np.uint32)
    msg = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    got = run(lib, ctxs, idx, form, wide, msg=msg)
    assert np.array_equal(got, oracle_sigs(oracle, orc_keys, idx, msg)), name


@pytest.mark.parametrize("form,wide,name", FORMS, ids=[f[2] for f in FORMS])
def test_pk_half_of_another_key(lib, oracle, orc_keys, form, wide, name):
    """a privKey whose pk half belongs to another seed: the signature hashes the given half, as the reference's does"""
    priv = orc_keys[:3].copy()
    priv[0, 32:] = orc_keys[4, 32:]
    priv[2, 32:] = np.arange(32, dtype=np.uint8)                         # not a point at all
    ctxs = init(lib, priv)
    idx = np.array([0, 1, 2, 0, 2, 1, 0], np.uint32)
    msg = np.random.default_rng(0x5c20).integers(0, 256, (len(idx), 33), dtype=np.uint8)
    assert np.array_equal(run(lib, ctxs, idx, form, wide, msg=msg), oracle_sigs(oracle, priv, idx, msg)), name


@pytest.mark.parametrize("form,wide,name", FORMS, ids=[f[2] for f in FORMS])
def test_foreign_contexts_against_the_model(lib, orc_keys, form, wide, name):
    """random-byte contexts (a any 256-bit value, bytes 96..127 not zero) and an honest context with a unclamped (bit 255 and low
    bits set): R = r*B, S = (h*a + r) mod L of the big-integer model"""
    rng = np.random.default_rng(0x5c30 + form * 2 + wide)
    ctxs = np.concatenate([rng.integers(0, 256, (3, CTX), dtype=np.uint8), init(lib, orc_keys[:2])])
    ctxs[3, 0] |= 7
    ctxs[3, 31] |= 0x80
    ctxs[4, :32] = 0xFF                                                    # a = 2^256 - 1
    idx = np.array([0, 1, 2, 3, 4, 2, 4, 0], np.uint32)
    msg = rng.integers(0, 256, (len(idx), 16), dtype=np.uint8)
    got = run(lib, ctxs, idx, form, wide, msg=msg)
    for i, k in enumerate(idx):
        assert got[i].tobytes() == model.sign_with_ctx(ctxs[k].tobytes(), msg[i].tobytes()), (name, i)


@pytest.mark.parametrize("form,wide,name", FORMS, ids=[f[2] for f in FORMS])
def test_message_lengths_at_the_block_edges(lib, oracle, orc_keys, form, wide, name):
    """ragged messages of 0, 47 | 48, 79 | 80, 175 | 176, 207 | 208 and 1000 bytes: both sides of each block edge of both hashes"""
    rng = np.random.default_rng(0x5c40 + form * 2 + wide)
    ctxs = init(lib, orc_keys)
    messages = [rng.integers(0, 256, m, dtype=np.uint8).tobytes() for m in EDGE_LENGTHS]
    idx = rng.integers(0, len(orc_keys), len(messages)).astype(np.uint32)
    got = run(lib, ctxs, idx, form, wide, messages=messages)
    assert np.array_equal(got, oracle_sigs(oracle, orc_keys, idx, messages)), name


@pytest.mark.parametrize("form,wide,name", FORMS, ids=[f[2] for f in FORMS])
def test_indices_at_and_past_the_end(lib, oracle, orc_keys, form, wide, name):
    """n_ctx - 1 signs like any other context; n_ctx and 0xffffffff give 64 zero bytes and leave their neighbours alone"""
    ctxs = init(lib, orc_keys)
    n_ctx = len(ctxs)
    idx = np.array([n_ctx - 1, n_ctx, 0xFFFFFFFF, 0, n_ctx, n_ctx - 1, 0xFFFFFFFF, 0x80000000, 1], np.uint32)
    msg = np.random.default_rng(0x5c50).integers(0, 256, (len(idx), 24), dtype=np.uint8)
    got = run(lib, ctxs, idx, form, wide, msg=msg)
    bad = idx >= n_ctx
    assert not got[bad].any(), name
    good = np.nonzero(~bad)[0]
    assert np.array_equal(got[good], oracle_sigs(oracle, orc_keys, idx[good], msg[good])), name
