"""GPU suite (MI355X): ed25519_ClassifyKey_*, ed25519_PublicKey_to_X25519_* and ed25519_PrivateKey_to_X25519_*.  Flags, ok and the
converted keys must be the bytes of the big-integer model of the stated rule (tests/key_model.py) on the case set the CPU tests
share, at every size and in both forms; the conversions must agree with the reference's own bytes (the golden key pairs, the
oracle's X25519 public key, hashlib) and must work as X25519 keys through curve25519_dh_Peer_Init_* and
curve25519_dh_CreateSharedKey_indexed_*."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import key_model as model
from curve25519_amd import _lib, synth
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 257, 1025, 4097, 65537)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_1024.npz")
FILL = 0xA5


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def cases():
    keys, labels = model.case_set()
    return keys, labels, model.expected(keys)


@pytest.fixture(scope="module")
def pool():
    """about 300 modelled keys, their expected outputs, and the rows that are edge cases (everything but the honest keys)"""
    keys = model.pool()
    flags, xpk, ok = model.expected(keys)
    edge = np.flatnonzero(flags != 11)
    assert 250 <= len(keys) <= 350 and len(edge) > 100
    return keys, flags, xpk, ok, edge


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def filled(shape, dtype):
    """a device tensor of `dtype` over shape[0] rows of shape[1] bytes, every byte FILL"""
    import torch
    t = torch.full(shape, FILL, dtype=torch.uint8, device=dev())
    return t if dtype == torch.uint8 else t.view(dtype)


def classify_dev(api, keys):
    import torch
    n = len(keys)
    d_flags = filled((n, 4), torch.int32)
    api.ed25519_ClassifyKey_dev(d_flags, to_dev(keys))
    torch.cuda.synchronize()
    return d_flags.cpu().numpy().view(np.uint32).reshape(n)


def convert_dev(api, keys):
    import torch
    n = len(keys)
    d_xpk, d_ok = filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
    api.ed25519_PublicKey_to_X25519_dev(d_xpk, d_ok, to_dev(keys))
    torch.cuda.synchronize()
    return d_xpk.cpu().numpy(), d_ok.cpu().numpy().reshape(n)


def private_dev(api, priv):
    import torch
    d_xsk = filled((len(priv), 32), torch.uint8)
    api.ed25519_PrivateKey_to_X25519_dev(d_xsk, to_dev(priv))
    torch.cuda.synchronize()
    return d_xsk.cpu().numpy()


def clamped_hash(seed: bytes) -> bytes:
    d = bytearray(hashlib.sha512(seed).digest()[:32])
    d[0] &= 248
    d[31] &= 127
    d[31] |= 64
    return bytes(d)


def test_case_set(api, cases):
    """the whole case set through _dev and _batch: the model's bytes, and both forms identical"""
    keys, labels, (flags, xpk, ok) = cases
    got = classify_dev(api, keys)
    bad = [(i, labels[i], keys[i].tobytes().hex(), int(got[i]), int(flags[i])) for i in np.flatnonzero(got != flags)]
    assert not bad, bad[:8]
    assert np.array_equal(api.ed25519_ClassifyKey(keys), flags)
    got_xpk, got_ok = convert_dev(api, keys)
    assert np.array_equal(got_ok, ok), [(i, labels[i]) for i in np.flatnonzero(got_ok != ok)][:8]
    assert np.array_equal(got_xpk, xpk), [(i, labels[i]) for i in np.flatnonzero((got_xpk != xpk).any(axis=1))][:8]
    host_xpk, host_ok = api.ed25519_PublicKey_to_X25519(keys)
    assert np.array_equal(host_xpk, xpk) and np.array_equal(host_ok, ok)
    assert set(int(f) for f in flags[np.array(labels) == "mixed order"]) == {3}, "the cases only the walk by L decides"


@pytest.mark.parametrize("n", SIZES)
def test_sizes(api, pool, n):
    """the pool tiled in a seeded permutation, edge cases in the first and last rows and on both sides of every 64-lane wave and
    256-lane workgroup boundary: every row is the model's, in both forms"""
    keys, flags, xpk, ok, edge = pool
    rng = np.random.default_rng(0x51 + n)
    idx = np.concatenate([rng.permutation(len(keys)) for _ in range(n // len(keys) + 1)])[:n]
    at = sorted({0, n - 1} | {p for b in range(64, n, 64) for p in (b - 1, b)})
    idx[at] = edge[(np.arange(len(at)) * 7 + n) % len(edge)]
    k = keys[idx]
    assert np.array_equal(classify_dev(api, k), flags[idx])
    got_xpk, got_ok = convert_dev(api, k)
    assert np.array_equal(got_ok, ok[idx]) and np.array_equal(got_xpk, xpk[idx])
    assert np.array_equal(api.ed25519_ClassifyKey(k), flags[idx])
    host_xpk, host_ok = api.ed25519_PublicKey_to_X25519(k)
    assert np.array_equal(host_ok, ok[idx]) and np.array_equal(host_xpk, xpk[idx])
    priv = synth.random_bytes((n, 64), 0x9000 + n)
    xsk = private_dev(api, priv)
    assert np.array_equal(xsk, api.ed25519_PrivateKey_to_X25519(priv))
    for i in sorted({0, n - 1, n // 2} | set(at[:6])):
        assert xsk[i].tobytes() == clamped_hash(priv[i, :32].tobytes()), i


def test_against_the_reference_bytes(api):
    """1,024 key pairs of the golden file: the converted public key is the X25519 public key of the converted private key, by this
    library's ladder and by the oracle's; the converted private key is the clamped hash, and what Sign_Init keeps in bytes 0..31"""
    z = np.load(GOLDEN)
    seeds = z["ed_sk"]
    assert seeds.shape == (1024, 32)
    pub, priv = api.ed25519_CreateKeyPair(seeds)
    assert np.array_equal(pub, z["ed_pub"]) and np.array_equal(priv, z["ed_priv"])
    xpk, ok = api.ed25519_PublicKey_to_X25519(pub)
    assert ok.all()
    xsk = api.ed25519_PrivateKey_to_X25519(priv)
    want_xsk = np.stack([np.frombuffer(clamped_hash(s.tobytes()), np.uint8) for s in seeds])
    assert np.array_equal(xsk, want_xsk)
    assert np.array_equal(xsk, api.ed25519_Sign_Init(priv)[:, :32])
    ours, clamped = api.curve25519_dh_CalculatePublicKey(xsk)
    assert np.array_equal(clamped, xsk), "already clamped"
    assert np.array_equal(xpk, ours)
    assert np.array_equal(xpk, Oracle().x25519_public(want_xsk)[0])
    assert np.array_equal(api.ed25519_ClassifyKey(pub), np.full(1024, 11, np.uint32))
    d_xpk, d_ok = convert_dev(api, pub)
    assert np.array_equal(d_xpk, xpk) and d_ok.all()
    assert np.array_equal(private_dev(api, priv), xsk)


def test_the_chain_works(api):
    """converted identities are X25519 keys: the two sides of a key agreement meet, directly and through Peer_Init and
    CreateSharedKey_indexed over 8 converted recipients"""
    pub, priv = api.ed25519_CreateKeyPair(synth.random_bytes((9, 32), 0xC4A1))
    xpk, ok = api.ed25519_PublicKey_to_X25519(pub)
    xsk = api.ed25519_PrivateKey_to_X25519(priv)
    assert ok.all()
    ab, _ = api.curve25519_dh_CreateSharedKey(xpk[1:2], xsk[0:1])
    ba, _ = api.curve25519_dh_CreateSharedKey(xpk[0:1], xsk[1:2])
    assert np.array_equal(ab, ba) and ab.any()
    # sender 0 seals to recipients 1..8 in one indexed call; each recipient opens with the sender's converted public key
    ctxs = api.curve25519_dh_Peer_Init(xpk[1:])
    idx = np.arange(8, dtype=np.uint32)
    sealed, _ = api.curve25519_dh_CreateSharedKey_indexed(ctxs, idx, np.repeat(xsk[0:1], 8, axis=0))
    opened, _ = api.curve25519_dh_CreateSharedKey(np.repeat(xpk[0:1], 8, axis=0), xsk[1:])
    assert np.array_equal(sealed, opened)
    assert len(set(r.tobytes() for r in sealed)) == 8 and sealed.any(axis=1).all()


def test_rejected_rows(api, cases):
    """a rejected key's row is 32 zero bytes and ok = 0, the rows around it are what they are without it, and every row of buffers
    pre-filled with 0xA5 is written"""
    keys, labels, (flags, xpk, ok) = cases
    lab = np.array(labels)
    honest = keys[lab == "honest"]
    rejected = keys[ok == 0]
    assert len(rejected) > 100 and {"mixed order", "small order", "off the curve", "y >= p"} <= set(lab[ok == 0])
    alone_xpk, alone_ok = convert_dev(api, honest)
    assert alone_ok.all() and alone_xpk.any(axis=1).all()
    n = 3 * len(rejected)
    mix = np.empty((n, 32), np.uint8)
    mix[0::3] = honest[np.arange(len(rejected)) % len(honest)]
    mix[1::3] = rejected
    mix[2::3] = honest[(np.arange(len(rejected)) + 1) % len(honest)]
    got_xpk, got_ok = convert_dev(api, mix)
    assert not got_xpk[1::3].any() and not got_ok[1::3].any()
    assert np.array_equal(got_xpk[0::3], alone_xpk[np.arange(len(rejected)) % len(honest)]) and (got_ok[0::3] == 1).all()
    assert np.array_equal(got_xpk[2::3], alone_xpk[(np.arange(len(rejected)) + 1) % len(honest)]) and (got_ok[2::3] == 1).all()
    got_flags = classify_dev(api, mix)
    assert (got_flags[0::3] == 11).all() and (got_flags[2::3] == 11).all() and np.array_equal(got_flags[1::3], flags[ok == 0])
    assert not (got_flags == 0xA5A5A5A5).any() and set(np.unique(got_ok)) == {0, 1}
    # all rejected: nothing but zeros, and still every row written
    got_xpk, got_ok = convert_dev(api, rejected)
    assert not got_xpk.any() and not got_ok.any()


def test_arguments(api, cases):
    """n == 0 returns 0 and writes nothing, a null pointer is an argument error, a call on another stream gives the same bytes"""
    import torch
    keys, labels, (flags, xpk, ok) = cases
    L = _lib.load()
    d_keys, d_priv = to_dev(keys), to_dev(synth.random_bytes((len(keys), 64), 0xA11))
    d_flags, d_xpk, d_ok = filled((4, 4), torch.int32), filled((4, 32), torch.uint8), filled((4, 4), torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.ed25519_ClassifyKey_dev(p(d_flags), p(d_keys), 0, None) == 0
    assert L.ed25519_PublicKey_to_X25519_dev(p(d_xpk), p(d_ok), p(d_keys), 0, None) == 0
    assert L.ed25519_PrivateKey_to_X25519_dev(p(d_xpk), p(d_priv), 0, None) == 0
    h_flags, h_xpk, h_ok = np.full(4, 0xA5A5A5A5, np.uint32), np.full((4, 32), FILL, np.uint8), np.full(4, 0x25A5A5A5, np.int32)
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    priv = synth.random_bytes((4, 64), 0xA12)
    assert L.ed25519_ClassifyKey_batch(hp(h_flags), hp(keys), 0) == 0
    assert L.ed25519_PublicKey_to_X25519_batch(hp(h_xpk), hp(h_ok), hp(keys), 0) == 0
    assert L.ed25519_PrivateKey_to_X25519_batch(hp(h_xpk), hp(priv), 0) == 0
    torch.cuda.synchronize()
    for t in (d_flags, d_xpk, d_ok):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()
    assert (h_flags == 0xA5A5A5A5).all() and (h_xpk == FILL).all() and (h_ok == 0x25A5A5A5).all()
    for rc in (L.ed25519_ClassifyKey_dev(None, p(d_keys), 4, None), L.ed25519_ClassifyKey_dev(p(d_flags), None, 4, None),
               L.ed25519_PublicKey_to_X25519_dev(None, p(d_ok), p(d_keys), 4, None),
               L.ed25519_PublicKey_to_X25519_dev(p(d_xpk), None, p(d_keys), 4, None),
               L.ed25519_PublicKey_to_X25519_dev(p(d_xpk), p(d_ok), None, 4, None),
               L.ed25519_PrivateKey_to_X25519_dev(None, p(d_priv), 4, None), L.ed25519_PrivateKey_to_X25519_dev(p(d_xpk), None, 4, None),
               L.ed25519_ClassifyKey_batch(None, hp(keys), 4), L.ed25519_ClassifyKey_batch(hp(h_flags), None, 4),
               L.ed25519_PublicKey_to_X25519_batch(None, hp(h_ok), hp(keys), 4),
               L.ed25519_PublicKey_to_X25519_batch(hp(h_xpk), None, hp(keys), 4),
               L.ed25519_PublicKey_to_X25519_batch(hp(h_xpk), hp(h_ok), None, 4),
               L.ed25519_PrivateKey_to_X25519_batch(None, hp(priv), 4), L.ed25519_PrivateKey_to_X25519_batch(hp(h_xpk), None, 4)):
        assert rc != 0 and b"null pointer" in L.c25519_amd_last_error()
    torch.cuda.synchronize()
    for t in (d_flags, d_xpk, d_ok):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all(), "a refused call writes nothing"
    base = torch.zeros(len(keys) * 32 + 16, dtype=torch.uint8, device=dev())
    assert L.ed25519_ClassifyKey_dev(p(d_flags), C.c_void_p(base.data_ptr() + 8), 4, None) != 0, "a misaligned device pointer is refused"
    side = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(side):
        n = len(keys)
        s_flags, s_xpk, s_ok = filled((n, 4), torch.int32), filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
        s_xsk = filled((n, 32), torch.uint8)
        api.ed25519_ClassifyKey_dev(s_flags, d_keys)
        api.ed25519_PublicKey_to_X25519_dev(s_xpk, s_ok, d_keys)
        api.ed25519_PrivateKey_to_X25519_dev(s_xsk, d_priv)
    side.synchronize()
    assert np.array_equal(s_flags.cpu().numpy().view(np.uint32).reshape(n), flags)
    assert np.array_equal(s_xpk.cpu().numpy(), xpk) and np.array_equal(s_ok.cpu().numpy().reshape(n), ok)
    assert np.array_equal(s_xsk.cpu().numpy(), private_dev(api, d_priv.cpu().numpy()))
