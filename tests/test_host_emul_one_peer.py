"""CPU tests of X25519 against ONE peer key over the peer's wide comb (curve25519_amd/csrc/x25519_peer.cuh: what
curve25519_dh_CreateSharedKey_one_peer_* runs on the device).  The device source is compiled by g++ against the C model of the
gfx950 primitives (tests/host_emul/one_peer.cpp, tests/host_emul/build.py's build_lib) and judged against a Python
big-integer ladder that reads u unmasked, and against the reference's own curve25519_dh_CreateSharedKey where it is built.
Every peer class: the known-answer keys, the small-order u, the twist and u = -1 (which must be refused), keys with bit 255
set, public keys of random secrets and random byte strings -- about half of the latter land on the curve WITH a torsion
component, the case the k >> 3 / 8P identity exists for."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import one_peer_cases as cases

vp, sz = C.c_void_p, C.c_size_t
SECRETS = 4                            # per peer


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_one_peer": ([vp, vp, vp, sz], C.c_int), "emul_one_peer_point": ([vp, vp], C.c_int),
                    "emul_one_peer_rows": ([vp, vp, vp, sz], None)},
                   "one_peer.cpp", "libc25519_emul_one_peer.so")
    yield lib
    assert_no_mad_overflow(lib)


def secrets(seed, n=SECRETS):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def one_peer(lib, pk: bytes, sk):
    sk = np.ascontiguousarray(sk, dtype=np.uint8).copy()
    out = np.zeros_like(sk)
    pkb = np.frombuffer(pk, np.uint8).copy()
    wide = lib.emul_one_peer(out.ctypes.data, pkb.ctypes.data, sk.ctypes.data, sk.shape[0])
    return out, sk, wide


def expect(pk: bytes, sk):
    out = np.array([np.frombuffer(cases.shared(pk, bytes(r)), np.uint8) for r in sk])
    clamped = np.array([np.frombuffer(cases.clamp(int.from_bytes(bytes(r), "little")).to_bytes(32, "little"), np.uint8) for r in sk])
    return out, clamped


def check_peers(lib, peers, seed, reference=None):
    walked = []
    for i, (name, pk) in enumerate(peers):
        sk = secrets(seed + i)
        got, got_sk, wide = one_peer(lib, pk, sk)
        exp, exp_sk = expect(pk, sk)
        assert np.array_equal(got, exp), name
        assert np.array_equal(got_sk, exp_sk), name
        assert wide == int(cases.eligible(int.from_bytes(pk, "little"))), name
        if reference is not None:
            ref, ref_sk = reference.x25519_shared(np.tile(np.frombuffer(pk, np.uint8), (len(sk), 1)), sk)
            assert np.array_equal(got, ref) and np.array_equal(got_sk, ref_sk), name
        if wide:
            walked.append(name)
    return walked


def test_fixed_peer_classes(lib):
    """KAT keys (0, 1, p - 1, p, p + 1, 2^255 - 1, 2^256 - 1, 9, p + 9, RFC 7748), small order, twist, u = -1, bit 255 set:
    the walk's bytes are the ladder's, and exactly the keys on the curve other than u = -1 walk the comb."""
    peers = cases.fixed_peers()
    walked = check_peers(lib, peers, 0x0e00)
    assert all(n in walked for n, _ in peers if n.startswith("small"))
    assert "bit255_on" in walked
    assert not any(n.startswith(("twist", "minus_one")) for n in walked)


def test_small_order_peers_give_zero(lib):
    """Q = 8P is the neutral element: the walk ends on a zero denominator, the shared key is 32 zero bytes, as from the ladder"""
    for u in cases.SMALL_ORDER:
        got, _, wide = one_peer(lib, cases.to_bytes(u), secrets(u & 0xffff))
        assert wide == 1 and not got.any(), u


def test_refused_peers(lib):
    """twist keys and u = -1 (mod p) are not eligible: k_x25519_peer_check's word is 0"""
    q = np.zeros(96, np.uint8)
    for u in (*cases.TWIST, *cases.MINUS_ONE):
        pk = np.frombuffer(cases.to_bytes(u), np.uint8).copy()
        assert lib.emul_one_peer_point(q.ctypes.data, pk.ctypes.data) == 0, u
    pk = np.frombuffer(cases.to_bytes(9), np.uint8).copy()
    assert lib.emul_one_peer_point(q.ctypes.data, pk.ctypes.data) == 1


def test_random_peers(lib):
    """~50 public keys of random secrets and ~50 random byte strings, a handful of secrets each; some of the byte strings
    carry a torsion component (L * P != O) and still come out right through k >> 3 and 8P"""
    peers = cases.random_peers(48, 0x0e01)
    walked = check_peers(lib, peers, 0x0e10)
    assert all(n in walked for n, _ in peers if n.startswith("pub"))
    torsion = [n for n, pk in peers if n in walked and n.startswith("raw") and cases.has_torsion(int.from_bytes(pk, "little"))]
    assert len(torsion) >= 10, torsion


def test_rows_in_the_device_layout(lib):
    """rows of a peer's comb in the layout k_x25519_peer_prepare writes: three canonical fields, then 2Z = 2 and zero padding"""
    q = np.zeros(96, np.uint8)
    pk = np.frombuffer(cases.to_bytes(9), np.uint8).copy()
    assert lib.emul_one_peer_point(q.ctypes.data, pk.ctypes.data) == 1
    idx = np.array([0, 4095, 4096, 3 * 4096 + 17], np.uint32)
    rows = np.zeros((len(idx), 32), np.uint32)
    lib.emul_one_peer_rows(rows.ctypes.data, q.ctypes.data, idx.ctypes.data, len(idx))
    assert (rows[:, 24] == 2).all() and not rows[:, 25:].any()
    assert len({bytes(r[:24]) for r in rows}) == len(idx)


def test_reference_agrees(lib, reference):
    """the reference's own curve25519_dh_CreateSharedKey on the same keys and secrets (where oracle/_ref is built)"""
    check_peers(lib, cases.fixed_peers() + cases.random_peers(8, 0x0e02), 0x0e20, reference=reference)
