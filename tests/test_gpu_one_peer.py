"""GPU suite (MI355X): curve25519_dh_CreateSharedKey_one_peer_* -- many secrets against ONE peer key, over a wide comb built
for 8 * the peer where the peer is on the curve.  Every output and every clamped secret must equal what
curve25519_dh_CreateSharedKey_dev gives with the key repeated n times, for every peer class (tests/one_peer_cases.py) and at the
sizes where the dispatch changes; c25519_amd_x25519_one_peer_last_wide must show that the comb really decided where it should
(otherwise a ladder-only implementation would pass every parity check)."""
import ctypes as C
import hashlib
import threading

import numpy as np
import pytest

import one_peer_cases as cases
from curve25519_amd import _lib, synth

pytestmark = pytest.mark.gpu

W = 3 << 15                           # the default ONE_PEER_WIDE (test_threshold_default pins it)
SIZES = (1, 63, 65, 4097, W - 1, W, W + 1, (1 << 17) + 3)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def u8(pk: bytes):
    return np.frombuffer(pk, np.uint8).reshape(1, 32).copy()


def last_wide():
    return _lib.load().c25519_amd_x25519_one_peer_last_wide()


def one_peer_dev(api, pk: bytes, sk):
    import torch
    dev = torch.device("cuda", 0)
    d_sk = torch.from_numpy(np.ascontiguousarray(sk)).to(dev)
    d_out = torch.empty_like(d_sk)
    api.curve25519_dh_CreateSharedKey_one_peer_dev(d_out, torch.from_numpy(u8(pk)).to(dev), d_sk)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_sk.cpu().numpy()


def ladder_dev(api, pk: bytes, sk):
    import torch
    dev = torch.device("cuda", 0)
    d_sk = torch.from_numpy(np.ascontiguousarray(sk)).to(dev)
    d_pk = torch.from_numpy(np.repeat(u8(pk), len(sk), axis=0)).to(dev)
    d_out = torch.empty_like(d_sk)
    api.curve25519_dh_CreateSharedKey_dev(d_out, d_pk, d_sk)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_sk.cpu().numpy()


def check(api, pk: bytes, sk, what=""):
    got, got_sk = one_peer_dev(api, pk, sk)
    wide = last_wide()
    exp, exp_sk = ladder_dev(api, pk, sk)
    assert np.array_equal(got, exp), (what, len(sk))
    assert np.array_equal(got_sk, exp_sk), (what, len(sk))
    return wide


def secrets(n, seed):
    return synth.random_bytes((n, 32), 0x0ee0000 + seed)


def peer_set():
    fixed = dict(cases.fixed_peers())
    rnd = dict(cases.random_peers(4, 0x0e30))
    torsion = next(pk for n, pk in rnd.items() if n.startswith("raw") and cases.eligible(int.from_bytes(pk, "little"))
                   and cases.has_torsion(int.from_bytes(pk, "little")))
    return {"pub": rnd["pub0"], "torsion": torsion, "kat": fixed["kat0"], "small": fixed["small2"], "twist": fixed["twist2"],
            "minus_one": fixed["minus_one0"], "bit255": fixed["bit255_on"]}


def test_every_size_equals_the_ladder(api):
    """each peer class at the sizes where the dispatch changes: per-wave kernels, quads, one lane per element, below / at / above
    ONE_PEER_WIDE, several pipeline pieces' worth; the comb walks from ONE_PEER_WIDE on for eligible peers"""
    _lib.load().c25519_amd_thread_release()
    for i, n in enumerate(SIZES):
        for name, pk in peer_set().items():
            wide = check(api, pk, secrets(n, 16 * i + len(name)), name)
            if n >= W:
                assert wide == int(cases.eligible(int.from_bytes(pk, "little"))), (name, n)


def test_every_peer_class_on_the_comb(api):
    """every fixed class and ~50 + ~50 random peers (public keys, random byte strings: some with a torsion component) with the comb
    built for each (ONE_PEER_WIDE = 1), 4097 secrets: the comb decides exactly the eligible ones, with the ladder's bytes"""
    with _lib.tunable("ONE_PEER_WIDE", 1):
        for j, (name, pk) in enumerate(cases.fixed_peers() + cases.random_peers(48, 0x0e31)):
            wide = check(api, pk, secrets(4097, 0x100 + j), name)
            assert wide == int(cases.eligible(int.from_bytes(pk, "little"))), name


def test_last_wide_reports_the_path(api):
    """1 for an on-curve peer from ONE_PEER_WIDE on, 1 again for the remembered peer below it; 0 for the twist, u = -1 and
    ONE_PEER_WIDE = 0; an ineligible peer does not evict the kept comb; -1 after the thread's state is released"""
    L = _lib.load()
    L.c25519_amd_thread_release()
    assert last_wide() == -1
    ps = peer_set()
    a = ps["pub"]
    assert check(api, a, secrets(W, 1)) == 1
    assert check(api, a, secrets(4097, 2)) == 1                 # remembered: any size above the per-wave range
    assert check(api, a, secrets(20000, 3)) == 1
    assert check(api, a, secrets(65, 4)) == 0                   # per-wave sizes run the ladder
    assert check(api, ps["twist"], secrets(W, 5)) == 0
    assert check(api, ps["minus_one"], secrets(W, 6)) == 0
    assert check(api, a, secrets(4097, 7)) == 1                 # ... and left the comb of `a` where it was
    assert check(api, ps["kat"], secrets(4097, 8)) == 0         # a new peer below the threshold: the ladder
    with _lib.tunable("ONE_PEER_WIDE", 0):
        assert check(api, a, secrets(W, 9)) == 0
    L.c25519_amd_thread_release()
    assert last_wide() == -1


def test_threshold_default(api):
    """with ONE_PEER_WIDE unset, a new eligible peer builds its comb at W secrets and not at W - 1"""
    assert _lib.load().c25519_amd_tunable_get(b"ONE_PEER_WIDE") == -1
    ps = peer_set()
    assert check(api, ps["pub"], secrets(W, 10)) == 1
    assert check(api, ps["torsion"], secrets(W - 1, 11)) == 0
    assert check(api, ps["torsion"], secrets(W, 12)) == 1


def test_no_stale_comb(api):
    """A -> B -> A, and two keys that differ only in bit 255: every call walks the comb of its own key or the ladder"""
    ps = peer_set()
    a, b = ps["pub"], ps["torsion"]
    c = bytearray(a)
    c[31] ^= 0x80
    c = bytes(c)
    for pk in (a, b, a, c, a, c):                               # builds each time
        assert check(api, pk, secrets(W, pk[0])) == int(cases.eligible(int.from_bytes(pk, "little")))
    kept = c if cases.eligible(int.from_bytes(c, "little")) else a     # (an ineligible key builds nothing)
    for pk in (a, c, b):                                        # below the threshold: only the kept comb is walked
        assert check(api, pk, secrets(4097, pk[1])) == int(pk == kept)
    assert check(api, b, secrets(W, 13)) == 1
    assert check(api, b, secrets(4097, 14)) == 1
    assert check(api, a, secrets(4097, 15)) == 0


def test_interleaved_with_one_key_verification(api):
    """one-key ed25519_Verify_Check and one-peer X25519 on one thread: each keeps its own comb"""
    L = _lib.load()
    esk = synth.random_bytes((1, 32), 0x0e40)
    pub, priv = api.ed25519_CreateKeyPair(esk)
    ctx = api.ed25519_Verify_Init(pub)[0]
    msg = synth.random_bytes((W, 32), 0x0e41)
    sig = api.ed25519_SignMessage(np.repeat(priv, W, axis=0), msg)
    bad = sig.copy()
    bad[::5, 40] ^= 1
    ok = api.ed25519_Verify_Check(ctx, bad, msg)
    assert L.c25519_amd_verify_check_last_wide() == 1
    assert np.array_equal(ok == 1, np.arange(W) % 5 != 0)
    pk = peer_set()["torsion"]
    assert check(api, pk, secrets(W, 20)) == 1
    ok = api.ed25519_Verify_Check(ctx, bad[:4096], msg[:4096])
    assert L.c25519_amd_verify_check_last_wide() == 1             # the verification comb survived the X25519 one
    assert np.array_equal(ok == 1, np.arange(4096) % 5 != 0)
    assert check(api, pk, secrets(4097, 21)) == 1                # ... and the other way round


def test_batch_form_and_threads(api):
    """the host-pointer form over several pipeline pieces, and two threads with different peers at once"""
    ps = peer_set()
    n = 3 * (1 << 16) + 5
    sk = secrets(n, 30)
    for pk in (ps["pub"], ps["twist"]):
        got, got_sk = api.curve25519_dh_CreateSharedKey_one_peer(u8(pk), sk)
        exp, exp_sk = api.curve25519_dh_CreateSharedKey(np.repeat(u8(pk), n, axis=0), sk)
        assert np.array_equal(got, exp) and np.array_equal(got_sk, exp_sk)
    errors = []
    peers = (ps["torsion"], ps["bit255"])
    work = [(pk, secrets(m, 40 + t)) for t, pk in enumerate(peers) for m in (W + 7, 5000)]
    expected = [api.curve25519_dh_CreateSharedKey(np.repeat(u8(pk), len(s), axis=0), s) for pk, s in work]

    def worker(t):
        try:
            for rep in range(3):
                for j in (2 * t, 2 * t + 1):
                    pk, s = work[j]
                    got, got_sk = api.curve25519_dh_CreateSharedKey_one_peer(u8(pk), s)
                    if not (np.array_equal(got, expected[j][0]) and np.array_equal(got_sk, expected[j][1])):
                        errors.append((t, rep, j))
                    if last_wide() != 1:
                        errors.append((t, rep, j, "ladder"))
            _lib.load().c25519_amd_thread_release()
        except Exception as e:                                  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert not errors, errors


def test_million_digest(api):
    """2^20 seeded secrets against one peer: the outputs' SHA-256 is the ladder's, device and host forms"""
    import torch
    n = 1 << 20
    sk = synth.random_bytes((n, 32), 0x0e50)
    pk = peer_set()["pub"]
    got, got_sk = one_peer_dev(api, pk, sk)
    assert last_wide() == 1
    exp, exp_sk = ladder_dev(api, pk, sk)
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    assert digest(got) == digest(exp) and digest(got_sk) == digest(exp_sk)
    host, host_sk = api.curve25519_dh_CreateSharedKey_one_peer(u8(pk), sk)
    assert digest(host) == digest(exp) and digest(host_sk) == digest(exp_sk)
    torch.cuda.synchronize()


def test_argument_errors(api):
    """a null pointer is an error code, n == 0 a no-op; the Python wrapper wants one key"""
    L = _lib.load()
    assert L.curve25519_dh_CreateSharedKey_one_peer_batch(None, None, None, 1) != 0
    assert L.curve25519_dh_CreateSharedKey_one_peer_batch(None, None, None, 0) != 0
    z = np.zeros((1, 32), np.uint8)
    assert L.curve25519_dh_CreateSharedKey_one_peer_batch(C.c_void_p(z.ctypes.data), C.c_void_p(z.ctypes.data), C.c_void_p(z.ctypes.data), 0) == 0
    with pytest.raises(ValueError):
        api.curve25519_dh_CreateSharedKey_one_peer(np.zeros((2, 32), np.uint8), np.zeros((2, 32), np.uint8))
