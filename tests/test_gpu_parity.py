"""GPU suite (pytest -m gpu, MI355X): the HIP path, called through the C-ABI of libcurve25519_amd.so, against
the committed golden fixtures (which hold the REAL reference's outputs) and against the oracle on seeded
inputs -- bit-exact everywhere, since every value on this path is an integer.

Sizes: known-answer vectors, the 1024-record fixture, config 1's N = 4096 and the full N = 2^20 batches of
configs 2-4 (digest of the reference's outputs + size-independent properties), ragged batch sizes
around the wave / workgroup widths, empty batches, message lengths around the SHA-512 block edges."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from curve25519_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KAT = json.load(open(os.path.join(GOLD, "kat.json")))
DIG = json.load(open(os.path.join(GOLD, "digests.json")))
R1024 = np.load(os.path.join(GOLD, "random_1024.npz"))
THREADS = min(os.cpu_count() or 1, int(os.environ.get("OMP_NUM_THREADS") or 0) or 1 << 30)   # a share of a big host: its thread budget
SHARED_GPU_MAX_PROCESSES = 6       # processes that may hold one device open at the same time (test_bench_self_launches_two_ranks)
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731


def h2a(s):
    return np.frombuffer(bytes.fromhex(s), np.uint8).reshape(1, -1)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def test_native_library_is_what_runs(api):
    """The extension must be the in-tree .so and must really be mapped into this process."""
    from curve25519_amd import _lib
    path = _lib.library_path()
    assert os.path.dirname(path) == os.path.join(ROOT, "curve25519_amd")
    api.curve25519_dh_CreateSharedKey(np.zeros((1, 32), np.uint8), np.ones((1, 32), np.uint8))
    assert "libcurve25519_amd.so" in open("/proc/self/maps").read()


def test_base_table_equals_reference_table(api, oracle):
    tbl = api.base_folding8_table()
    assert sha(tbl) == KAT["base_folding8_sha256"]
    assert np.array_equal(tbl, oracle.base_table())


def test_field_layer_against_big_integers(api):
    """L0 unit test (the reference's ECP_SELF_TEST field identities, test/curve25519_selftest.c:640-741): the
    device field ops on adversarial 256-bit patterns against Python big-integer arithmetic mod p."""
    from curve25519_amd import _lib
    import vectors
    L = _lib.load()
    pairs, a, b = vectors.field_cases()
    n = len(pairs)
    for op in vectors.FIELD_OPS:
        bb = b
        if op in vectors.FIELD_OPS_B_REDUCED:                # contract: the subtrahend is a reduced element
            bb = np.stack([vectors.le(y % vectors.P, 32) for _, y in pairs])
        out = np.empty((n, 32), np.uint8)
        assert L.c25519_amd_fe_selftest(out.ctypes.data, a.ctypes.data, bb.ctypes.data, n, op) == 0
        vectors.check_field(op, out, pairs)
    # 1 / x three ways (op 4: what the kernels run; 12: x^(p-2); 13: division steps) on the wider set of inversion patterns
    pairs, a, b = vectors.inversion_cases()
    for op in (4, 12, 13, 14):
        out = np.empty((len(pairs), 32), np.uint8)
        assert L.c25519_amd_fe_selftest(out.ctypes.data, a.ctypes.data, b.ctypes.data, len(pairs), op) == 0
        vectors.check_field(op, out, pairs)


def test_scalar_layer_borrow_paths(api):
    """mod-L unit test on the device (the reference's eco_* checks, test/curve25519_selftest.c:624-714): n*L +- 1,
    b*R +- 1, all-ones digests -- the inputs on which sc_reduce_hi / sc_mod take their add-back paths, which hashed
    inputs reach with probability ~2^-95."""
    from curve25519_amd import _lib
    import vectors
    L = _lib.load()
    a512, b256, a, b = vectors.scalar_cases()
    n = len(a512)
    for op in vectors.SCALAR_OPS:
        out = np.empty((n, 32), np.uint8)
        assert L.c25519_amd_sc_selftest(out.ctypes.data, a.ctypes.data, b.ctypes.data, n, op) == 0
        vectors.check_scalar(op, out, a512, b256)


def test_fold_recodings_match_the_reference(api):
    """ecp_8Folds / ecp_4Folds outputs of the reference (KAT["folds"]) against the device's three recoders."""
    from curve25519_amd import _lib
    L = _lib.load()
    recs = KAT["folds"]
    k = np.concatenate([h2a(r["k"]) for r in recs])
    k = np.ascontiguousarray(np.concatenate([k] * 9)[:130])          # more than two waves
    out = np.empty((k.shape[0], 128), np.uint8)
    assert L.c25519_amd_fold_selftest(out.ctypes.data, k.ctypes.data, k.shape[0]) == 0
    for i in range(k.shape[0]):
        r = recs[i % len(recs)]
        assert out[i, :32].tobytes().hex() == r["fold8"] and out[i, 32:64].tobytes().hex() == r["fold8"]
        assert out[i, 64:].tobytes().hex() == r["fold4"]


# ---- known-answer vectors -------------------------------------------------------------------------------

def test_x25519_kats(api):
    recs = KAT["x25519"]
    pk = np.concatenate([h2a(r["pk"]) for r in recs])
    sk = np.concatenate([h2a(r["sk"]) for r in recs])
    shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
    for i, r in enumerate(recs):
        assert shared[i].tobytes().hex() == r["shared"], r["name"]
        assert clamped[i].tobytes().hex() == r["sk_clamped"], r["name"]


def test_x25519_public_kats(api):
    recs = KAT["x25519_public"]
    sk = np.concatenate([h2a(r["sk"]) for r in recs])
    for fast in (False, True):
        pk, clamped = api.curve25519_dh_CalculatePublicKey(sk, fast=fast)
        for i, r in enumerate(recs):
            assert pk[i].tobytes().hex() == r["pk"], (r["name"], fast)
            assert clamped[i].tobytes().hex() == r["sk_clamped"]


def test_ed25519_kats_all_message_lengths(api):
    for r in KAT["ed25519"]:                        # message lengths 0..257 -> one batch of one per length
        msg = np.frombuffer(bytes.fromhex(r["msg"]), np.uint8).reshape(1, -1)
        pub, priv = api.ed25519_CreateKeyPair(h2a(r["sk"]))
        assert pub.tobytes().hex() == r["pk"] and priv.tobytes().hex() == r["priv"], r["name"]
        sig = api.ed25519_SignMessage(priv, msg)
        assert sig.tobytes().hex() == r["sig"], r["name"]
        assert int(api.ed25519_VerifySignature(sig, pub, msg)[0]) == 1, r["name"]


def test_ed25519_verify_quirks(api):
    """Negative vectors and the reference's non-RFC behaviour: S+L accepted, no key validation."""
    for r in KAT["ed25519_verify"]:
        msg = np.frombuffer(bytes.fromhex(r["msg"]), np.uint8).reshape(1, -1)
        got = int(api.ed25519_VerifySignature(h2a(r["sig"]), h2a(r["pk"]), msg)[0])
        assert got == r["verify"], r["name"]


# ---- fixtures with the reference's outputs --------------------------------------------------------------

def test_random_1024_fixture(api):
    g = R1024
    shared, clamped = api.curve25519_dh_CreateSharedKey(g["x_pk"], g["x_sk"])
    assert np.array_equal(shared, g["x_shared"]) and np.array_equal(clamped, g["x_sk_clamped"])
    pub, priv = api.ed25519_CreateKeyPair(g["ed_sk"])
    assert np.array_equal(pub, g["ed_pub"]) and np.array_equal(priv, g["ed_priv"])
    assert np.array_equal(api.ed25519_SignMessage(priv, g["ed_msg"]), g["ed_sig"])
    assert np.array_equal(api.ed25519_VerifySignature(g["v_sig"], pub, g["v_msg"]), g["v_ok"])


def gpu_digests(api, n):
    sk, pk = synth.x25519_inputs(n)
    shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
    esk, msg = synth.ed25519_inputs(n)
    pub, priv = api.ed25519_CreateKeyPair(esk)
    sig = api.ed25519_SignMessage(priv, msg)
    bsig, bmsg, bad = synth.corrupt_for_verify(sig, msg)
    ok = api.ed25519_VerifySignature(bsig, pub, bmsg)
    assert np.array_equal(ok == 0, bad), "exactly the corrupted entries are rejected"
    return {"n": n, "x25519_shared": sha(shared), "x25519_sk_clamped": sha(clamped), "ed25519_pub": sha(pub),
            "ed25519_priv": sha(priv), "ed25519_sig": sha(sig), "ed25519_verdicts": sha(ok.astype("<i4")),
            "verify_rejected": int(bad.sum())}


@pytest.mark.parametrize("n", [k for k in ("1024", "4096", str(1 << 20)) if k in DIG])
def test_seeded_batches_hash_to_the_reference_digests(api, n):
    """BASELINE.json configs 1-4 at their real sizes: outputs of the HIP path hash to the digests of the
    reference's outputs on the same seeded inputs."""
    assert gpu_digests(api, int(n)) == DIG[n]


# ---- against the oracle: ragged sizes, edge inputs -------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_ragged_batch_sizes(api, oracle, n):
    sk = synth.random_bytes((n, 32), 0xA000 + n)
    pk = synth.random_bytes((n, 32), 0xB000 + n)
    msg = synth.random_bytes((n, 24), 0xC000 + n)
    shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
    e_shared, e_clamped = oracle.x25519_shared(pk, sk, threads=THREADS)
    assert np.array_equal(shared, e_shared) and np.array_equal(clamped, e_clamped)
    pub, priv = api.ed25519_CreateKeyPair(sk)
    e_pub, e_priv = oracle.ed25519_keypair(sk, threads=THREADS)
    assert np.array_equal(pub, e_pub) and np.array_equal(priv, e_priv)
    sig = api.ed25519_SignMessage(priv, msg)
    assert np.array_equal(sig, oracle.ed25519_sign(priv, msg, threads=THREADS))
    if n:
        sig[::2, 40] ^= 1
    ok = api.ed25519_VerifySignature(sig, pub, msg)
    assert np.array_equal(ok, oracle.ed25519_verify(sig, pub, msg, threads=THREADS))
    assert ok.shape == (n,)


def test_edge_public_keys_and_garbage(api, oracle):
    P = 2**255 - 19
    vals = [0, 1, 2, 9, P - 1, P, P + 1, P + 9, 2**255 - 1, 2**255, 2**255 + 9, 2**256 - 1, 2**256 - 20]
    pk = np.stack([np.frombuffer(int(v).to_bytes(32, "little"), np.uint8) for v in vals] * 5)
    sk = synth.random_bytes((pk.shape[0], 32), 0xED6E)
    shared, _ = api.curve25519_dh_CreateSharedKey(pk, sk)
    assert np.array_equal(shared, oracle.x25519_shared(pk, sk)[0])
    assert not shared[0].any() and not shared[1].any()            # low-order inputs -> zero bytes
    # Ed25519 verify on unvalidated garbage keys / signatures must give the reference's verdicts
    n = 2048
    gs, gp, gm = synth.random_bytes((n, 64), 31), synth.random_bytes((n, 32), 32), synth.random_bytes((n, 32), 33)
    gp[: len(vals)] = pk[: len(vals)]
    assert np.array_equal(api.ed25519_VerifySignature(gs, gp, gm), oracle.ed25519_verify(gs, gp, gm, threads=THREADS))


@pytest.mark.parametrize("mlen", [0, 1, 3, 8, 47, 48, 49, 63, 64, 65, 111, 112, 113, 128, 300, 1021, 5000])
def test_message_lengths(api, oracle, mlen):
    n = 130
    sk = synth.random_bytes((n, 32), 0x5000 + mlen)
    msg = synth.random_bytes((n, mlen), 0x6000 + mlen)
    pub, priv = oracle.ed25519_keypair(sk, threads=THREADS)
    sig = api.ed25519_SignMessage(priv, msg)
    assert np.array_equal(sig, oracle.ed25519_sign(priv, msg, threads=THREADS))
    assert api.ed25519_VerifySignature(sig, pub, msg).all()
    if mlen:
        msg[:, mlen - 1] ^= 0x80
        assert not api.ed25519_VerifySignature(sig, pub, msg).any()


def test_ragged_message_lengths(api, oracle):
    """Per-element message lengths in one batch (the reference takes msg_size per call): lengths 0..300 mixed."""
    n = 700
    sk = synth.random_bytes((n, 32), 0x8001)
    pub, priv = oracle.ed25519_keypair(sk, threads=THREADS)
    lens = synth.random_bytes((n, 2), 0x8002).astype(np.int64)
    lens = (lens[:, 0] * 256 + lens[:, 1]) % 301
    lens[:8] = [0, 1, 47, 48, 111, 112, 128, 300]
    blob = synth.random_bytes((int(lens.sum()) + 1,), 0x8003)
    offs = np.concatenate([[0], np.cumsum(lens)])
    msgs = [blob[offs[i]:offs[i + 1]].tobytes() for i in range(n)]
    sig = api.ed25519_SignMessage_ragged(priv, msgs)
    exp = np.concatenate([oracle.ed25519_sign(priv[i:i + 1], np.frombuffer(msgs[i], np.uint8).reshape(1, -1))
                          for i in range(n)])
    assert np.array_equal(sig, exp)
    assert api.ed25519_VerifySignature_ragged(sig, pub, msgs).all()
    bad = [m + b"x" if i % 3 == 0 else m for i, m in enumerate(msgs)]
    ok = api.ed25519_VerifySignature_ragged(sig, pub, bad)
    assert np.array_equal(ok == 0, np.arange(n) % 3 == 0)


# ---- size-independent properties at the full batch size --------------------------------------------------

def test_full_size_properties(api):
    n = 1 << 20
    a = synth.random_bytes((n, 32), 0x1111)
    b = synth.random_bytes((n, 32), 0x2222)
    pa, _ = api.curve25519_dh_CalculatePublicKey(a, fast=True)
    pb, _ = api.curve25519_dh_CalculatePublicKey(b)
    s1, _ = api.curve25519_dh_CreateSharedKey(pb, a)
    s2, _ = api.curve25519_dh_CreateSharedKey(pa, b)
    assert np.array_equal(s1, s2), "a*(b*G) == b*(a*G) for every lane (8-fold walk vs ladder on one side)"
    assert s1.any(axis=1).all()
    msg = synth.random_bytes((n, 32), 0x3333)
    pub, priv = api.ed25519_CreateKeyPair(a)
    sig = api.ed25519_SignMessage(priv, msg)
    assert api.ed25519_VerifySignature(sig, pub, msg).all(), "sign -> verify round trip"
    assert not api.ed25519_VerifySignature(sig, np.roll(pub, 1, axis=0), msg).any(), "wrong key rejects"


@pytest.mark.parametrize("n", [65535, 65536, 65537, 131072, 131073, 262144, 262145])
def test_workgroup_shapes_at_their_boundaries(api, oracle, n, monkeypatch):
    """A *_dev call picks its kernel shape from n (X25519: the one-launch kernel in 64-lane workgroups up to 2^16 elements,
    ladder + shared inversion as two launches beyond; the tunable XF_SPLIT = 0 / 1 forces either, the one-launch kernel then in
    64 / 128 / 256 / 512 lanes up to 2^16 / 2^17 / 2^18 / beyond with an inversion per 1 / 2 / 4 / 8 elements; the
    fixed-base kernels 256 / 512 / 1024 lanes): every shape, at the sizes where it changes and with a ragged last
    workgroup, gives the reference's bytes."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sk_np = synth.random_bytes((n, 32), 0xD000 + n % 977)
    pk_np = synth.random_bytes((n, 32), 0xE000 + n % 977)
    msg_np = synth.random_bytes((n, 20), 0xF000 + n % 977)
    pk_np[7] = 0                                                      # a low-order point: its Z is 0 in a shared inversion
    sk, pk, msg = up(sk_np), up(pk_np), up(msg_np)
    shared = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    skc = sk.clone()
    api.curve25519_dh_CreateSharedKey_dev(shared, pk, skc)
    e_shared, e_clamped = oracle.x25519_shared(pk_np, sk_np, threads=THREADS)
    assert np.array_equal(shared.cpu().numpy(), e_shared) and np.array_equal(skc.cpu().numpy(), e_clamped)
    from curve25519_amd import _lib
    for forced in (0, 1):                                             # the shape the default did not pick at this n, too
        with _lib.tunable("XF_SPLIT", forced):
            shared.zero_()
            skc = sk.clone()
            api.curve25519_dh_CreateSharedKey_dev(shared, pk, skc)
            assert np.array_equal(shared.cpu().numpy(), e_shared) and np.array_equal(skc.cpu().numpy(), e_clamped), forced
    pub = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    priv = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    api.ed25519_CreateKeyPair_dev(pub, priv, sk)
    e_pub, e_priv = oracle.ed25519_keypair(sk_np, threads=THREADS)
    assert np.array_equal(pub.cpu().numpy(), e_pub) and np.array_equal(priv.cpu().numpy(), e_priv)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    api.ed25519_SignMessage_dev(sig, priv, msg)
    assert np.array_equal(sig.cpu().numpy(), oracle.ed25519_sign(e_priv, msg_np, threads=THREADS))
    ok = torch.empty((n, 1), dtype=torch.int32, device=dev)
    sig[::3, 33] ^= 4
    api.ed25519_VerifySignature_dev(ok, sig, pub, msg)
    assert np.array_equal(ok.cpu().numpy().reshape(-1), oracle.ed25519_verify(sig.cpu().numpy(), e_pub, msg_np, threads=THREADS))


def test_large_odd_batch(api, oracle):
    """n = 2^22 + 77 (not a multiple of any tile, 4x the benchmark batch): index arithmetic, scratch carving and
    the batched-inversion tail.  Checked by properties plus an oracle spot check of the first / last rows."""
    n = (1 << 22) + 77
    a = synth.random_bytes((n, 32), 0x4441)
    b = synth.random_bytes((n, 32), 0x4442)
    pa, _ = api.curve25519_dh_CalculatePublicKey(a, fast=True)
    pb, _ = api.curve25519_dh_CalculatePublicKey(b, fast=True)
    s1, _ = api.curve25519_dh_CreateSharedKey(pb, a)
    s2, _ = api.curve25519_dh_CreateSharedKey(pa, b)
    assert np.array_equal(s1, s2)
    rows = np.r_[0:64, n - 64:n]
    assert np.array_equal(s1[rows], oracle.x25519_shared(pb[rows], a[rows])[0])
    msg = synth.random_bytes((n, 16), 0x4443)
    pub, priv = api.ed25519_CreateKeyPair(a)
    sig = api.ed25519_SignMessage(priv, msg)
    assert np.array_equal(sig[rows], oracle.ed25519_sign(priv[rows], msg[rows]))
    ok = api.ed25519_VerifySignature(sig, pub, msg)
    assert ok.all()
    sig[n - 1, 0] ^= 1
    assert api.ed25519_VerifySignature(sig[n - 200:], pub[n - 200:], msg[n - 200:]).sum() == 199


# ---- the other faces of the boundary --------------------------------------------------------------------

def test_device_pointer_entry_points(api, oracle):
    import torch
    n = 3000
    dev = torch.device("cuda", 0)
    sk_np, pk_np = synth.x25519_inputs(n)
    sk, pk = torch.from_numpy(sk_np).to(dev), torch.from_numpy(pk_np).to(dev)
    out = torch.empty_like(pk)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        api.curve25519_dh_CreateSharedKey_dev(out, pk, sk)
    s.synchronize()
    e_out, e_sk = oracle.x25519_shared(pk_np, sk_np, threads=THREADS)
    assert np.array_equal(out.cpu().numpy(), e_out) and np.array_equal(sk.cpu().numpy(), e_sk)
    api.curve25519_dh_CreateSharedKey_dev(pk, pk, sk)              # shared may alias pk
    torch.cuda.synchronize()
    assert np.array_equal(pk.cpu().numpy(), e_out)
    from curve25519_amd import _lib
    with pytest.raises(_lib.EngineError):                           # misaligned device pointer is refused
        api.curve25519_dh_CreateSharedKey_dev(out[: n - 1], out.view(-1)[1:32 * (n - 1) + 1].view(n - 1, 32), sk[: n - 1])


def test_operations_on_several_streams_overlap_safely(api, oracle):
    """A thread that issues X25519, signing and verification on different streams gets a work-scratch slab per stream
    (up to four per device; a fifth stream reuses the least recently used one behind an event): the calls may overlap on
    the device and every result equals the one-stream result.  Six streams, three rounds, two sizes per operation, so
    slabs are shared, regrown and handed from stream to stream while kernels are in flight."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    n = 40000
    sk_np, pk_np = synth.x25519_inputs(n)
    esk, msg = synth.ed25519_inputs(n)
    e_shared, _ = oracle.x25519_shared(pk_np, sk_np, threads=THREADS)
    pub_np, priv_np = api.ed25519_CreateKeyPair(esk)
    sig_np = api.ed25519_SignMessage(priv_np, msg)
    bsig, bmsg, bad = synth.corrupt_for_verify(sig_np, msg)
    pub_np = pub_np.copy()
    pub_np[5::1000] = synth.random_bytes((len(pub_np[5::1000]), 32), 0x51de)      # garbage keys: the slow list, per stream
    e_ok = oracle.ed25519_verify(bsig, pub_np, bmsg, threads=THREADS)
    d = dict(sk=up(sk_np), pk=up(pk_np), priv=up(priv_np), msg=up(msg), bsig=up(bsig), pub=up(pub_np), bmsg=up(bmsg))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in range(6)]
    results = []
    for rnd in range(3):
        for j, st in enumerate(streams):
            m = n if (j + rnd) & 1 else n // 3                       # different sizes: slabs of different capacity
            with torch.cuda.stream(st):
                kind = (j + rnd) % 3
                if kind == 0:
                    out = torch.empty((m, 32), dtype=torch.uint8, device=dev)
                    api.curve25519_dh_CreateSharedKey_dev(out, d["pk"][:m], d["sk"][:m].clone())
                elif kind == 1:
                    out = torch.empty((m, 64), dtype=torch.uint8, device=dev)
                    api.ed25519_SignMessage_dev(out, d["priv"][:m], d["msg"][:m])
                else:
                    out = torch.empty((m, 1), dtype=torch.int32, device=dev)
                    api.ed25519_VerifySignature_dev(out, d["bsig"][:m], d["pub"][:m], d["bmsg"][:m])
                results.append((kind, m, out))
    torch.cuda.synchronize()
    for kind, m, out in results:
        want = (e_shared, sig_np, np.asarray(e_ok).reshape(-1, 1))[kind][:m]
        assert np.array_equal(out.cpu().numpy().reshape(want.shape), want), (kind, m)


def test_two_phase_verification(api, oracle):
    """ed25519_Verify_Init once per key, many ed25519_Verify_Check (reference ed25519_verify.c:282-286):
    same verdicts as the one-shot path and as the oracle; the context has the reference's 2080-byte shape."""
    nk, n = 5, 3000
    sk = synth.random_bytes((nk, 32), 0x7001)
    pub, priv = oracle.ed25519_keypair(sk)
    ctx = api.ed25519_Verify_Init(pub)
    assert ctx.shape == (nk, 2080) and np.array_equal(ctx[:, :32], pub)
    one = (1).to_bytes(32, "little")
    for k in range(nk):                                   # row 0 is the neutral element (1, 1, 0, 2)
        assert ctx[k, 32:64].tobytes() == one and ctx[k, 64:96].tobytes() == one
        assert not ctx[k, 96:128].any() and ctx[k, 128:160].tobytes() == (2).to_bytes(32, "little")
    for k in range(nk):
        msg = synth.random_bytes((n, 40), 0x7100 + k)
        sig = oracle.ed25519_sign(np.repeat(priv[k:k + 1], n, axis=0), msg, threads=THREADS)
        sig[::7, 3] ^= 0x20
        msg[1::7, 39] ^= 1
        sig[2::7, 33] ^= 2
        got = api.ed25519_Verify_Check(ctx[k], sig, msg)
        exp = oracle.ed25519_verify(sig, np.repeat(pub[k:k + 1], n, axis=0), msg, threads=THREADS)
        assert np.array_equal(got, exp)
        assert np.array_equal(got, api.ed25519_VerifySignature(sig, np.repeat(pub[k:k + 1], n, axis=0), msg))
        assert 0 < got.sum() < n
    # garbage keys: Verify_Init never rejects.  For off-curve inputs the table VALUES depend on the order of the
    # doublings / additions, so comparing them with the oracle pins the device's operation sequence.
    gp = synth.random_bytes((4, 32), 0x7200)
    gctx = api.ed25519_Verify_Init(gp)
    P = 2**255 - 19
    for keys, ctxs in ((gp, gctx), (pub, ctx)):
        exp = oracle.verify_init_table(keys)
        for k in range(keys.shape[0]):
            rows = ctxs[k, 32:].reshape(16, 4, 32)
            got = [[int.from_bytes(rows[r, f].tobytes(), "little") for f in range(4)] for r in range(16)]
            assert all(v < P for row in got for v in row)        # device rows are canonical
            for r in range(16):                                  # equal as PROJECTIVE points (Y+X : Y-X : 2dT : 2Z)
                g, e = got[r], exp[k][r]
                for f in range(3):
                    assert (g[f] * e[3] - e[f] * g[3]) % P == 0, (k, r, f)
                assert (g[3] == 0) == (e[3] == 0)
    # calls of a few keys / pairs run one operation per wave (k_ed25519_verify_init_coop, _check_coop): the same BYTES as the
    # per-lane kernels' contexts (the one-key fast path recognises a context by them) and the same verdicts
    from curve25519_amd import _lib
    with _lib.tunable("COOP_MAX", 0):
        assert np.array_equal(api.ed25519_Verify_Init(gp), gctx) and np.array_equal(api.ed25519_Verify_Init(pub), ctx)
    gs, gm = synth.random_bytes((256, 64), 0x7201), synth.random_bytes((256, 16), 0x7202)
    for k in range(4):
        with _lib.tunable("COOP_MAX", 0):
            per_lane = api.ed25519_Verify_Check(gctx[k], gs, gm)
        assert np.array_equal(api.ed25519_Verify_Check(gctx[k], gs, gm), per_lane)
        assert np.array_equal(api.ed25519_Verify_Check(gctx[k], gs, gm),
                              oracle.ed25519_verify(gs, np.repeat(gp[k:k + 1], 256, axis=0), gm))


def test_one_key_batches_walk_two_wide_combs_with_the_reference_verdicts(api, oracle):
    """ed25519_Verify_Check over a BIG batch under one key (the reference's amortisation: Verify_Init once, many Verify_Check,
    ed25519_verify.c:282-286) evaluates T = s*B + h*(-A) over two wide fixed-base combs -- the base point's and one built for
    -A on the spot (k_ed25519_verify_ctx_prepare / _check_wide) -- when the context is Verify_Init's own and the key is on
    the curve; any other context keeps the reference-order kernel.  Same verdicts as that kernel (tunable ONE_KEY_WIDE = 0) and
    as the oracle for: honest keys with corrupted entries and S + L; every small-order key (torsion: an even h must not
    become h + L) with the degenerate-but-valid vectors the real reference accepts for it; a mixed-order key; an off-curve
    key; a context with one byte changed (which the reference-order kernel reads as it is)."""
    from curve25519_amd import _lib
    import vectors
    n = (1 << 16) + 37
    rng_sig, rng_msg = synth.random_bytes((n, 64), 0x7301), synth.random_bytes((n, 24), 0x7302)
    d = np.load(os.path.join(GOLD, "degenerate_verify.npz"))
    dsig, dpk, dmsg, dver = (np.ascontiguousarray(d[k]) for k in ("sig", "pk", "msg", "verdict"))

    def both_paths(ctx, sig, msg):
        wide = api.ed25519_Verify_Check(ctx, sig, msg)
        with _lib.tunable("ONE_KEY_WIDE", 0):
            ref_order = api.ed25519_Verify_Check(ctx, sig, msg)
        assert np.array_equal(wide, ref_order), int((wide != ref_order).sum())
        return wide

    # honest keys
    sk = synth.random_bytes((2, 32), 0x7303)
    pub, priv = oracle.ed25519_keypair(sk)
    ctx = api.ed25519_Verify_Init(pub)
    for k in range(2):
        msg = rng_msg.copy()
        sig = oracle.ed25519_sign(np.repeat(priv[k:k + 1], n, axis=0), msg, threads=THREADS)
        sig[::7, 3] ^= 0x20
        msg[1::7, 23] ^= 1
        sig[2::7, 33] ^= 2
        for i in range(3, 600, 7):                                      # S + L: accepted by the reference
            S = int.from_bytes(sig[i, 32:].tobytes(), "little")
            if S + vectors.L < 2**256:
                sig[i, 32:] = vectors.le(S + vectors.L, 32)
        got = both_paths(ctx[k], sig, msg)
        assert np.array_equal(got, oracle.ed25519_verify(sig, np.repeat(pub[k:k + 1], n, axis=0), msg, threads=THREADS))
        assert n // 2 < got.sum() < n
    # small-order and mixed-order keys: every degenerate vector of the fixture (8-byte messages) under its own key, inside a
    # batch of garbage signatures for that key -- the real reference's verdicts where the fixture has them, the oracle's elsewhere
    sig8, msg8 = synth.random_bytes((n, 64), 0x7304), synth.random_bytes((n, dmsg.shape[1]), 0x7305)
    valid_seen = 0
    for key in np.unique(dpk, axis=0):
        at = np.nonzero((dpk == key).all(axis=1))[0]
        sig, msg = sig8.copy(), msg8.copy()
        pos = np.arange(len(at)) * 13 + 5
        sig[pos], msg[pos] = dsig[at], dmsg[at]
        cx = api.ed25519_Verify_Init(key.reshape(1, 32))[0]
        got = both_paths(cx, sig, msg)
        assert np.array_equal(got[pos], dver[at]), key.tobytes().hex()
        assert np.array_equal(got, oracle.ed25519_verify(sig, np.repeat(key.reshape(1, 32), n, axis=0), msg, threads=THREADS)), key.tobytes().hex()
        valid_seen += int(dver[at].sum())
    assert valid_seen == int(dver.sum()) > 300
    # an off-curve key, and a context somebody wrote into: the reference-order kernel decides, reading the rows as they are
    off = next(k for k in synth.random_bytes((64, 32), 0x999) if vectors.ed_decode(int.from_bytes(k.tobytes(), "little") & (2**255 - 1), 0) is None)
    cx = api.ed25519_Verify_Init(off.reshape(1, 32))[0]
    got = both_paths(cx, rng_sig, rng_msg)
    assert np.array_equal(got, oracle.ed25519_verify(rng_sig, np.repeat(off.reshape(1, 32), n, axis=0), rng_msg, threads=THREADS))
    msg = rng_msg.copy()
    sig = oracle.ed25519_sign(np.repeat(priv[:1], n, axis=0), msg, threads=THREADS)
    tampered = ctx[0].copy()
    tampered[32 + 128 * 5 + 7] ^= 0x40                                   # one byte of row 5
    honest = both_paths(ctx[0], sig, msg)
    assert honest.all()
    bent = both_paths(tampered, sig, msg)
    assert not bent.all()                                                # about one signature in sixteen meets row 5 with a nonzero ... and fails
    # the key's comb is remembered between calls (one Verify_Init, many Verify_Check): the same context again, another key in
    # between, the first one again, a tampered copy of the remembered context -- each call gets its own key's verdicts
    sig_b = oracle.ed25519_sign(np.repeat(priv[1:2], n, axis=0), msg, threads=THREADS)
    for cx, sg, want_all in ((ctx[0], sig, True), (ctx[0], sig, True), (ctx[1], sig_b, True), (ctx[1], sig, False), (ctx[0], sig, True),
                             (tampered, sig, False), (ctx[0], sig, True)):
        got = api.ed25519_Verify_Check(cx, sg, msg)
        assert bool(got.all()) == want_all and (want_all or got.sum() < n // 8)
    # ... and on two streams of one thread, two keys alternating, nothing synchronised in between (the kept buffer follows the
    # work slabs' stream-order rule)
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_ctx, d_sig, d_msg = [up(ctx[0]), up(ctx[1])], [up(sig), up(sig_b)], up(msg)
    outs = [torch.full((n, 1), -1, dtype=torch.int32, device=dev) for _ in range(6)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    L = _lib.load()
    for j in range(6):
        k = j & 1
        _lib.check(L.ed25519_Verify_Check_dev(C.c_void_p(outs[j].data_ptr()), C.c_void_p(d_ctx[k].data_ptr()), C.c_void_p(d_sig[k].data_ptr()),
                                              C.c_void_p(d_msg.data_ptr()), msg.shape[1], n, C.c_void_p(streams[(j // 2) & 1].cuda_stream)),
                   "ed25519_Verify_Check_dev")
    torch.cuda.synchronize()
    assert all(bool((o == 1).all().item()) for o in outs)
    # small batches stay on the reference-order kernel unless asked (ONE_KEY_WIDE = 1: every batch)
    with _lib.tunable("ONE_KEY_WIDE", 1):
        assert np.array_equal(api.ed25519_Verify_Check(ctx[0], sig[:300], msg[:300]), honest[:300])


def test_concurrent_host_threads(api, oracle):
    """The shim is re-entrant like the reference (SURVEY.md 8(b) Threading): host threads calling the batch API
    at the same time each get their own stream, staging buffers and scratch."""
    import threading
    results, errors = {}, []

    def worker(t):
        try:
            n = 3000 + 257 * t
            sk = synth.random_bytes((n, 32), 0x9000 + t)
            pk = synth.random_bytes((n, 32), 0x9100 + t)
            msg = synth.random_bytes((n, 20 + t), 0x9200 + t)
            for _ in range(3):
                shared, _ = api.curve25519_dh_CreateSharedKey(pk, sk)
                pub, priv = api.ed25519_CreateKeyPair(sk)
                sig = api.ed25519_SignMessage(priv, msg)
                ok = api.ed25519_VerifySignature(sig, pub, msg)
            results[t] = (sk, pk, msg, shared, pub, sig, ok)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, (sk, pk, msg, shared, pub, sig, ok) in results.items():
        assert np.array_equal(shared, oracle.x25519_shared(pk, sk, threads=THREADS)[0]), t
        epub, epriv = oracle.ed25519_keypair(sk, threads=THREADS)
        assert np.array_equal(pub, epub) and np.array_equal(sig, oracle.ed25519_sign(epriv, msg, threads=THREADS)), t
        assert ok.all()


def test_verify_point_on_garbage_keys(api, oracle):
    """The point T = s*B + h*(-A) itself (not just the 0/1 verdict) for unvalidated garbage keys and signatures:
    off the curve its value depends on the exact order of the walk's doublings and additions, so equality with
    the oracle pins the device's Verify_Check sequence, which a verdict of 0 == 0 cannot."""
    import ctypes as C
    import torch
    from curve25519_amd import _lib
    L = _lib.load()
    n = 1500
    sig = synth.random_bytes((n, 64), 0xA501)
    pk = synth.random_bytes((n, 32), 0xA502)
    msg = synth.random_bytes((n, 24), 0xA503)
    good_sk = synth.random_bytes((100, 32), 0xA504)                 # a valid stretch in the middle
    gpub, gpriv = oracle.ed25519_keypair(good_sk)
    pk[200:300] = gpub
    sig[200:300] = oracle.ed25519_sign(gpriv, msg[200:300])
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(a).to(dev) for a in (sig, pk, msg)]
    out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    _lib.check(L.c25519_amd_verify_point_dev(C.c_void_p(out.data_ptr()), C.c_void_p(d[0].data_ptr()),
                                             C.c_void_p(d[1].data_ptr()), C.c_void_p(d[2].data_ptr()), 24, n, None),
               "c25519_amd_verify_point_dev")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    exp = oracle.ed25519_verify_point(sig, pk, msg)
    assert np.array_equal(got, exp)
    assert np.array_equal(got[200:300], sig[200:300, :32])            # valid signatures: T encodes to R


def test_single_call_reference_api(api):
    """The eleven reference entry points, one element at a time (a device batch of one each)."""
    from curve25519_amd import _lib
    L = _lib.load()
    buf = lambda b: (C.c_ubyte * len(b)).from_buffer_copy(b)  # noqa: E731
    r = next(x for x in KAT["x25519"] if x["name"] == "rfc7748-1")
    sk, pk, out = buf(bytes.fromhex(r["sk"])), buf(bytes.fromhex(r["pk"])), (C.c_ubyte * 32)()
    L.curve25519_dh_CreateSharedKey(out, pk, sk)
    assert bytes(out).hex() == r["shared"] and bytes(sk).hex() == r["sk_clamped"]
    r = KAT["x25519_public"][0]
    for fn in (L.curve25519_dh_CalculatePublicKey, L.curve25519_dh_CalculatePublicKey_fast):
        sk = buf(bytes.fromhex(r["sk"]))
        fn(out, sk)
        assert bytes(out).hex() == r["pk"]
    r = next(x for x in KAT["ed25519"] if x["name"] == "rfc8032-test3")
    pub, priv, sig = (C.c_ubyte * 32)(), (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
    msg = bytes.fromhex(r["msg"])
    L.ed25519_CreateKeyPair(pub, priv, None, buf(bytes.fromhex(r["sk"])))
    L.ed25519_SignMessage(sig, priv, None, buf(msg), len(msg))
    assert bytes(pub).hex() == r["pk"] and bytes(sig).hex() == r["sig"]
    assert L.ed25519_VerifySignature(sig, pub, buf(msg), len(msg)) == 1
    ctx = L.ed25519_Verify_Init(None, pub)
    assert L.ed25519_Verify_Check(ctx, sig, buf(msg), len(msg)) == 1
    assert L.ed25519_Verify_Check(ctx, sig, buf(b"xx"), 2) == 0
    L.ed25519_Verify_Finish(ctx)


def test_c_caller_links_and_passes(tmp_path):
    """A plain C program written against the reference's two public headers, linked to this library."""
    exe = str(tmp_path / "dropin_test")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "dropin_test.c"), "-o", exe,
                           "-L", os.path.join(ROOT, "curve25519_amd"), "-lcurve25519_amd",
                           "-Wl,-rpath," + os.path.join(ROOT, "curve25519_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failure(s)" in p.stdout


def test_exit_with_a_call_in_flight(tmp_path):
    """The process calls exit() while another thread is in the middle of *_batch (and *_multi) calls: with a CPU library that is
    harmless; here a kernel launch into a HIP runtime that exit() is tearing down was a segmentation fault inside libamdhip64.
    The entry points now hold a gate (capi_common.hpp: ApiCall): the library's atexit handler closes it and waits for the calls
    in flight; a thread that calls again is parked.  tests/c/exit_midcall.c must exit 0 every time, at several points of the loop."""
    exe = str(tmp_path / "exit_midcall")
    subprocess.check_call(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "exit_midcall.c"),
                           "-o", exe, "-L", os.path.join(ROOT, "curve25519_amd"), "-lcurve25519_amd", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "curve25519_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    for mode in (0, 1):
        for us in (300, 1100, 2300, 4100, 7700, 13000):        # (a call takes 2-4 ms: every phase of one gets its turn)
            p = subprocess.run([exe, str(mode), str(us)], capture_output=True, text=True, timeout=60)
            assert p.returncode == 0, (mode, us, p.returncode, p.stderr[-1500:])


def test_reference_harness_runs_on_this_library():
    """The reference's own test/curve25519_test.c (dh_test, signature_test with the RFC 8032 vector and the
    blinded path, the donna cross-check and speed_test), built in the build container by
    `make -C oracle ref-harness` against libcurve25519_amd.so instead of libcurve25519.a.  Its exit code is its
    failure count.  Skipped where the prebuilt binary did not travel."""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_harness_on_amd")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_harness_on_amd not built (needs /root/reference at build time)")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "Signature Verified Successfully" in p.stdout
    assert "FAILED" not in p.stdout


def test_reference_cxx_wrappers_run_on_this_library():
    """the reference's C++ classes (C++/x25519.cpp: DH + SHA-512 KDF; C++/ed25519.cpp: keygen / sign
    with the reference's static blinding contexts, verify), compiled where they lie by `make -C oracle ref-cxx` and
    linked against libcurve25519_amd.so, reproduce the RFC 7748 / RFC 8032 vectors.  Exit code = failure count."""
    exe = os.path.join(ROOT, "oracle", "_ref", "cxx_wrappers_on_amd")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/cxx_wrappers_on_amd not built (needs /root/reference at build time)")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert "0 failure(s)" in p.stdout and "FAIL" not in p.stdout


def test_blinding_contexts_are_real_and_output_neutral(api, oracle):
    """ed25519_Blinding_Init builds (bl, zr, BP) on the device; signing / key generation with it walk the scalar
    k + bl and add BP, and the bytes are those of the unblinded calls (reference ed25519_sign.c:254-259; its harness
    asserts the same equality, test/curve25519_test.c:385-394)."""
    from curve25519_amd import _lib
    import vectors
    L = _lib.load()
    n = 5000
    sk, msg = synth.random_bytes((n, 32), 0xB101), synth.random_bytes((n, 45), 0xB102)
    pub, priv = api.ed25519_CreateKeyPair(sk)
    sig = api.ed25519_SignMessage(priv, msg)
    assert np.array_equal(sig, oracle.ed25519_sign(priv, msg, threads=THREADS))
    ctxs = []
    for seed in (b"", b"x", bytes(range(64)), bytes(200)):
        ctx = np.zeros(192, np.uint8)
        sbuf = np.frombuffer(seed, np.uint8).copy() if seed else np.zeros(1, np.uint8)
        got = L.ed25519_Blinding_Init(ctx.ctypes.data, sbuf.ctypes.data, len(seed))
        assert got == ctx.ctypes.data                       # caller's storage is filled, as in the reference
        bl = int.from_bytes(ctx[:32].tobytes(), "little")
        assert 0 < bl < vectors.L and ctx[32:64].any() and ctx[160:192].tobytes() == (2).to_bytes(32, "little")
        ctxs.append(ctx.tobytes())
        bpub, bpriv = np.empty_like(pub), np.empty_like(priv)
        _lib.check(L.ed25519_CreateKeyPair_blinded_batch(bpub.ctypes.data, bpriv.ctypes.data, ctx.ctypes.data,
                                                         sk.ctypes.data, n), "keypair blinded")
        assert np.array_equal(bpub, pub) and np.array_equal(bpriv, priv)
        bsig = np.empty_like(sig)
        _lib.check(L.ed25519_SignMessage_blinded_batch(bsig.ctypes.data, priv.ctypes.data, ctx.ctypes.data,
                                                       msg.ctypes.data, msg.shape[1], n), "sign blinded")
        assert np.array_equal(bsig, sig)
    assert len(set(ctxs)) == 4
    # the single-call API with a malloc'ed context
    L.ed25519_Blinding_Init.restype = C.c_void_p
    h = L.ed25519_Blinding_Init(None, b"seed", 4)
    one_pub, one_priv, one_sig = (C.c_ubyte * 32)(), (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
    L.ed25519_CreateKeyPair(one_pub, one_priv, C.c_void_p(h), sk[0].ctypes.data)
    L.ed25519_SignMessage(one_sig, one_priv, C.c_void_p(h), msg[0].ctypes.data, msg.shape[1])
    L.ed25519_Blinding_Finish(C.c_void_p(h))
    assert bytes(one_pub) == pub[0].tobytes() and bytes(one_sig) == sig[0].tobytes()


@pytest.mark.parametrize("comb", [0, 1])
def test_fixed_base_combs_give_the_reference_bytes(api, oracle, comb):
    """Both shapes of the fixed-base walk (tunable BASE_COMB; edp_BasePointMultiply, ed25519_sign.c:215-268): 0 = the 8 x 32
    signed comb staged in 120 KiB of LDS, 1 = the wide 13 x 20 comb whose rows a lane fetches through L2 by its column number
    (as the reference indexes its table, :239-243).  Whichever is the default, each is forced here: the 2^20 digests of the
    reference's key pairs and signatures, X25519 public keys against the ladder, ragged sizes around the workgroup
    shapes, blinded calls, and the table test hook (which the wide comb's tables must not disturb)."""
    from curve25519_amd import _lib
    L = _lib.load()
    with _lib.tunable("BASE_COMB", comb), _lib.tunable("COOP_MAX", 0):       # the batch kernels at every size
        n = 1 << 20
        esk, msg = synth.ed25519_inputs(n)
        pub, priv = api.ed25519_CreateKeyPair(esk)
        sig = api.ed25519_SignMessage(priv, msg)
        d = DIG[str(n)]
        assert (sha(pub), sha(priv), sha(sig)) == (d["ed25519_pub"], d["ed25519_priv"], d["ed25519_sig"])
        sk = synth.random_bytes((70001, 32), 0xC0B + comb)
        sk[0], sk[1] = 0, 0xff
        fast, c1 = api.curve25519_dh_CalculatePublicKey(sk, fast=True)
        slow, c2 = api.curve25519_dh_CalculatePublicKey(sk)
        assert np.array_equal(fast, slow) and np.array_equal(c1, c2)
        for m in (1, 255, 256, 257, 4097):
            p2, q2 = api.ed25519_CreateKeyPair(esk[:m])
            assert np.array_equal(p2, pub[:m]) and np.array_equal(q2, priv[:m]), m
            m37 = synth.random_bytes((m, 37), 0xC1B + m)
            assert np.array_equal(api.ed25519_SignMessage(priv[:m], m37), oracle.ed25519_sign(priv[:m], m37)), m
        ctx = np.zeros(192, np.uint8)
        seed = np.frombuffer(b"comb", np.uint8).copy()
        assert L.ed25519_Blinding_Init(ctx.ctypes.data, seed.ctypes.data, len(seed)) == ctx.ctypes.data
        m = 5000
        bpub, bpriv, bsig = np.empty((m, 32), np.uint8), np.empty((m, 64), np.uint8), np.empty((m, 64), np.uint8)
        _lib.check(L.ed25519_CreateKeyPair_blinded_batch(bpub.ctypes.data, bpriv.ctypes.data, ctx.ctypes.data, esk.ctypes.data, m), "keypair blinded")
        assert np.array_equal(bpub, pub[:m]) and np.array_equal(bpriv, priv[:m])
        _lib.check(L.ed25519_SignMessage_blinded_batch(bsig.ctypes.data, priv.ctypes.data, ctx.ctypes.data, msg.ctypes.data, 32, m), "sign blinded")
        assert np.array_equal(bsig, sig[:m])
    tbl = np.empty((256, 96), np.uint8)
    _lib.check(L.c25519_amd_base_table(tbl.ctypes.data), "c25519_amd_base_table")
    assert sha(tbl) == KAT["base_folding8_sha256"]


def test_dev_entry_points_validate_their_pointers(api):
    """*_dev calls refuse host memory and misaligned pointers instead of faulting inside a kernel."""
    import torch
    from curve25519_amd import _lib
    L = _lib.load()
    dev = torch.device("cuda", 0)
    n = 256
    d = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    h = np.zeros((n, 32), np.uint8)
    rc = L.curve25519_dh_CreateSharedKey_dev(C.c_void_p(d.data_ptr()), C.c_void_p(h.ctypes.data), C.c_void_p(d.data_ptr()), n, None)
    assert rc != 0 and b"device pointers" in L.c25519_amd_last_error()
    rc = L.ed25519_VerifySignature_dev(C.c_void_p(h.ctypes.data), C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()),
                                       C.c_void_p(d.data_ptr()), 16, n // 2, None)
    assert rc != 0
    with pytest.raises(ValueError):                                  # the torch wrappers check shapes first
        api.curve25519_dh_CreateSharedKey_dev(d, d[: n - 1], d)
    with pytest.raises(ValueError):
        api.ed25519_VerifySignature_dev(torch.zeros((n, 1), dtype=torch.int64, device=dev), torch.zeros((n, 64), dtype=torch.uint8, device=dev), d, d)


def test_thread_resources_are_released(api):
    """Per-thread streams / staging / scratch are freed on thread exit and by c25519_amd_thread_release(): a churn of
    short-lived threads must not grow device memory (round-1 leaked ~2.7 KB per verified element per thread)."""
    import threading
    import torch
    from curve25519_amd import _lib
    L = _lib.load()
    n = 1 << 15
    sk, msg = synth.random_bytes((n, 32), 0xC001), synth.random_bytes((n, 32), 0xC002)
    pub, priv = api.ed25519_CreateKeyPair(sk)
    sig = api.ed25519_SignMessage(priv, msg)

    def work():
        assert api.ed25519_VerifySignature(sig, pub, msg).all()

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
    assert free_a - free_b < 16 << 20, (free_a, free_b)    # one verify scratch alone is ~90 MB at this n
    work()                                                  # and the main thread still works after its own release


def test_mixed_config5_through_hip_engine(api):
    """BASELINE.json configs[4] at one GPU's share (2^20 mixed, contiguous thirds) through sharded.mixed_sharded and
    the HIP engine with a process group of one rank: every third equals the same rows of the full 2^20 batches, whose
    SHA-256 digests are the reference's (DIG) -- so the mixed path is tied to the reference's outputs."""
    import torch
    import torch.distributed as dist
    from curve25519_amd import sharded
    n = 1 << 20
    dev = torch.device("cuda", 0)
    eng = sharded.HipEngine(dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    sk, pk = synth.x25519_inputs(n)
    esk, msg = synth.ed25519_inputs(n)
    full_shared = eng.x25519_shared(up(pk), up(sk)).cpu().numpy()
    pub, priv = eng.ed25519_keypair(up(esk))
    sig = eng.ed25519_sign(priv, up(msg))
    bsig, bmsg, bad = synth.corrupt_for_verify(sig.cpu().numpy(), msg)
    full_ok = eng.ed25519_verify(up(bsig), pub, up(bmsg)).cpu().numpy()
    d = DIG[str(n)]
    assert sha(full_shared) == d["x25519_shared"] and sha(sig.cpu().numpy()) == d["ed25519_sig"]
    assert sha(full_ok.reshape(-1).astype("<i4")) == d["ed25519_verdicts"]
    (xa, xb), (sa, sb), (va, vb) = sharded.mixed_thirds(n)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        m_shared, m_sig, m_ok = sharded.mixed_sharded(
            eng, up(pk[xa:xb]), up(sk[xa:xb]), priv[sa:sb].contiguous(), up(msg[sa:sb]),
            up(bsig[va:vb]), pub[va:vb].contiguous(), up(bmsg[va:vb]))
        # the one-collective form bench.py uses (RCCL gather, world of one)
        og = sharded.OverlappedGather(xb - xa, 32, dev, root=0)
        buf = og.next_buffer()
        buf.copy_(m_shared)
        og.submit()
        og.finish()
        assert torch.equal(og.gathered(0), m_shared)
    finally:
        dist.destroy_process_group()
    assert np.array_equal(m_shared.cpu().numpy(), full_shared[xa:xb])
    assert np.array_equal(m_sig.cpu().numpy(), sig.cpu().numpy()[sa:sb])
    assert np.array_equal(m_ok.cpu().numpy(), full_ok[va:vb])
    assert np.array_equal(m_ok.cpu().numpy().reshape(-1) == 0, bad[va:vb])


def test_bench_mixed_and_self_launch_run():
    """bench.py --workload mixed (configs[4]) prints a well-formed line, and the N>1 code path (process group, RCCL
    gathers) runs with a world of one rank."""
    for extra in (["--workload", "mixed"], ["--dist-selftest", "--no-side"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu"] + extra,
                           capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-3000:]
        assert len(p.stdout.strip().splitlines()) == 1, p.stdout          # exactly one line on stdout
        line = json.loads(p.stdout)
        assert line["n_gpus"] == 1 and line["value"] > 0 and line["roofline"]["frac"] > 0
        assert line["roofline"]["binding"] == "valu" and 0.3 < line["roofline"]["binding_frac"] < 1.0
        # what the run timed is bit-exact against the reference's digests (2^20 per GPU: committed for every rank)
        assert line["bit_exact"]["all"] is True and line["bit_exact"]["mismatch"] is False, line["bit_exact"]
        if "mixed" in extra:
            assert line["verify_rejects_exactly_the_corrupted"] is True
            assert set(line["roofline"]["parts"]) == {"x25519", "sign", "verify"}
            assert [line["bit_exact"][k] for k in ("x25519", "sign", "verify")] == [True] * 3
        else:
            assert line["bit_exact"]["gathered_rows_at_root"] == {"x25519": [True]}     # the rows RCCL delivered to the root


def test_reference_openssl_harness_runs_on_this_library():
    """The reference's second-opinion harness, test/openssl_test.c, compiled where it lies by `make -C oracle ref-openssl`
    and linked against libcurve25519_amd.so + libcrypto: the key pair, public key, shared key and signature of OpenSSL's
    X25519 / Ed25519 against this library's single-call drop-in API, byte for byte (its memcmp at :218-226).  Exit code =
    number of mismatching operations."""
    exe = os.path.join(ROOT, "oracle", "_ref", "openssl_test_on_amd")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/openssl_test_on_amd not built (needs /root/reference and libcrypto at build time)")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "Mismatched" not in p.stdout and p.stdout.count("ratio") == 4


@pytest.mark.parametrize("force_gather,gather_mode", [(False, 1), (True, 1), (True, 0)])
def test_c_abi_multi_device_entry_points(api, force_gather, gather_mode, monkeypatch):
    """The C-level multi-GPU entry points (one worker thread and pinned pipeline per device, grouped ncclGather of the
    result rows to devices[0], segment by segment, a drain thread on the root) with EVERY device this box has: on a
    multi-GPU node that is a real RCCL communicator over xGMI, on a one-GPU box a communicator of one rank -- the shard /
    worker / segment / gather / hand-over code is the same for any count.  Results are the fixture's (the reference's)
    bytes; sizes that do not divide by the device count included.  A one-device handle normally skips the gather (its own
    rows would come back); force_gather makes it take the N > 1 path anyway (two segments for the big batch), and
    c25519_amd_multi_set_gather(h, 0) switches the gather off again: every device downloads its own rows."""
    from curve25519_amd import _lib
    L = _lib.load()
    _lib.set_tunable("MULTI_FORCE_GATHER", 1 if force_gather else -1)
    ndev = min(api.device_count(), 8)
    devs = (C.c_int * ndev)(*range(ndev))
    h = C.c_void_p()
    _lib.check(L.c25519_amd_multi_create(C.byref(h), devs, ndev), "c25519_amd_multi_create")
    try:
        assert L.c25519_amd_multi_device_count(h) == ndev
        _lib.check(L.c25519_amd_multi_set_gather(h, gather_mode), "c25519_amd_multi_set_gather")
        g = {k: np.ascontiguousarray(R1024[k]) for k in R1024.files}     # materialise once: ctypes gets raw pointers
        for n in (1024, 1000, 1023, ndev, 1):
            sk, pk = g["x_sk"][:n].copy(), g["x_pk"][:n].copy()
            shared = np.empty((n, 32), np.uint8)
            _lib.check(L.curve25519_dh_CreateSharedKey_multi(h, shared.ctypes.data, pk.ctypes.data, sk.ctypes.data, n), "x25519 multi")
            assert np.array_equal(shared, g["x_shared"][:n]) and np.array_equal(sk, g["x_sk_clamped"][:n])
            sig = np.empty((n, 64), np.uint8)
            priv, msg = np.ascontiguousarray(g["ed_priv"][:n]), np.ascontiguousarray(g["ed_msg"][:n])
            _lib.check(L.ed25519_SignMessage_multi(h, sig.ctypes.data, priv.ctypes.data, msg.ctypes.data, 32, n), "sign multi")
            assert np.array_equal(sig, g["ed_sig"][:n])
            ok = np.empty(n, np.int32)
            vs, vm, pub = np.ascontiguousarray(g["v_sig"][:n]), np.ascontiguousarray(g["v_msg"][:n]), np.ascontiguousarray(g["ed_pub"][:n])
            _lib.check(L.ed25519_VerifySignature_multi(h, ok.ctypes.data, vs.ctypes.data, pub.ctypes.data, vm.ctypes.data, 32, n), "verify multi")
            assert np.array_equal(ok, g["v_ok"][:n])
        assert L.curve25519_dh_CreateSharedKey_multi(h, shared.ctypes.data, g["x_pk"].ctypes.data, sk.ctypes.data, 0) == 0
        # a batch big enough for every device's pipeline to run in pieces (2^17 per device and more), against the
        # single-GPU host-pointer path on the same arrays
        n = (1 << 17) * ndev + 1000
        sk, pk = synth.x25519_inputs(n)
        sk2 = sk.copy()
        a, b = np.empty((n, 32), np.uint8), np.empty((n, 32), np.uint8)
        _lib.check(L.curve25519_dh_CreateSharedKey_multi(h, a.ctypes.data, pk.ctypes.data, sk.ctypes.data, n), "x25519 multi (big)")
        _lib.check(L.curve25519_dh_CreateSharedKey_batch(b.ctypes.data, pk.ctypes.data, sk2.ctypes.data, n), "x25519 batch (big)")
        assert np.array_equal(a, b) and np.array_equal(sk, sk2)
        # ... and the two Ed25519 operations at that size (64-byte rows and int32 verdicts through the segments)
        esk, msg = synth.ed25519_inputs(n)
        pub, priv = api.ed25519_CreateKeyPair(esk)
        s1, s2 = np.empty((n, 64), np.uint8), np.empty((n, 64), np.uint8)
        _lib.check(L.ed25519_SignMessage_multi(h, s1.ctypes.data, priv.ctypes.data, msg.ctypes.data, 32, n), "sign multi (big)")
        _lib.check(L.ed25519_SignMessage_batch(s2.ctypes.data, priv.ctypes.data, msg.ctypes.data, 32, n), "sign batch (big)")
        assert np.array_equal(s1, s2)
        vsig, vmsg, bad = synth.corrupt_for_verify(s1, msg)
        ok = np.full(n, -1, np.int32)
        _lib.check(L.ed25519_VerifySignature_multi(h, ok.ctypes.data, vsig.ctypes.data, pub.ctypes.data, vmsg.ctypes.data, 32, n), "verify multi (big)")
        assert np.array_equal(ok == 0, bad) and set(np.unique(ok)) <= {0, 1}
    finally:
        L.c25519_amd_multi_destroy(h)
        _lib.set_tunable("MULTI_FORCE_GATHER", -1)
    bad = (C.c_int * 1)(63)
    assert L.c25519_amd_multi_create(C.byref(h), bad, 1) != 0


@pytest.mark.parametrize("gather_mode", [1, 0])
def test_multi_device_code_with_eight_virtual_devices(api, gather_mode):
    """The D > 1 code of the *_multi entry points on a box with ONE GPU: a device list that names device 0 eight times runs
    eight workers, shards, pipelines and gather streams on it -- everything of the 8-GPU path except RCCL itself (which
    refuses a duplicate device; the gather of a piece is then eight device-to-device copies): uneven shards (n = 8k + 5:
    five devices own one row more, the others send a zeroed pad row), pieces cut at the same rows on every device, the
    rank-major blocks of a gathered piece, the drain / copier hand-over through the pinned slots, and the helper-thread
    budget (on real devices the same code calls ncclGather, rccl.h:745).  Bit-exact against the fixture
    (the reference's bytes) and against the single-GPU host-pointer path at 2^20."""
    from curve25519_amd import _lib
    L = _lib.load()
    devs = (C.c_int * 8)(*([0] * 8))
    h = C.c_void_p()
    _lib.check(L.c25519_amd_multi_create(C.byref(h), devs, 8), "c25519_amd_multi_create (8 x device 0)")
    try:
        assert L.c25519_amd_multi_device_count(h) == 8
        _lib.check(L.c25519_amd_multi_set_gather(h, gather_mode), "c25519_amd_multi_set_gather")
        # the threads that copy memory while a call runs fit the CPUs this process may use (not the host's thread count)
        assert 0 < L.c25519_amd_multi_helper_threads(h) <= max(L.c25519_amd_usable_cpus(), 8 + 2)
        g = {k: np.ascontiguousarray(R1024[k]) for k in R1024.files}
        for n in (1021, 8, 5, 1):                                      # 8k + 5; one row each; fewer rows than devices
            sk, pk = g["x_sk"][:n].copy(), g["x_pk"][:n].copy()
            shared = np.empty((n, 32), np.uint8)
            _lib.check(L.curve25519_dh_CreateSharedKey_multi(h, shared.ctypes.data, pk.ctypes.data, sk.ctypes.data, n), "x25519 multi")
            assert np.array_equal(shared, g["x_shared"][:n]) and np.array_equal(sk, g["x_sk_clamped"][:n]), n
            sig = np.empty((n, 64), np.uint8)
            priv, msg = np.ascontiguousarray(g["ed_priv"][:n]), np.ascontiguousarray(g["ed_msg"][:n])
            _lib.check(L.ed25519_SignMessage_multi(h, sig.ctypes.data, priv.ctypes.data, msg.ctypes.data, 32, n), "sign multi")
            assert np.array_equal(sig, g["ed_sig"][:n]), n
            ok = np.empty(n, np.int32)
            vs, vm, pub = np.ascontiguousarray(g["v_sig"][:n]), np.ascontiguousarray(g["v_msg"][:n]), np.ascontiguousarray(g["ed_pub"][:n])
            _lib.check(L.ed25519_VerifySignature_multi(h, ok.ctypes.data, vs.ctypes.data, pub.ctypes.data, vm.ctypes.data, 32, n), "verify multi")
            assert np.array_equal(ok, g["v_ok"][:n]), n
        # 2^20 + 5: every virtual device's pipeline runs in pieces (2^17 rows each), shards uneven; digests of the reference
        n = (1 << 20) + 5
        sk, pk = synth.x25519_inputs(n)
        sk2 = sk.copy()
        a, b = np.empty((n, 32), np.uint8), np.empty((n, 32), np.uint8)
        _lib.check(L.curve25519_dh_CreateSharedKey_multi(h, a.ctypes.data, pk.ctypes.data, sk.ctypes.data, n), "x25519 multi (2^20 + 5)")
        assert sha(a[: 1 << 20]) == DIG[str(1 << 20)]["x25519_shared"] and sha(sk[: 1 << 20]) == DIG[str(1 << 20)]["x25519_sk_clamped"]
        _lib.check(L.curve25519_dh_CreateSharedKey_batch(b.ctypes.data, pk.ctypes.data, sk2.ctypes.data, n), "x25519 batch")
        assert np.array_equal(a, b) and np.array_equal(sk, sk2)
        esk, msg = synth.ed25519_inputs(n)
        pub, priv = api.ed25519_CreateKeyPair(esk)
        s1 = np.empty((n, 64), np.uint8)
        _lib.check(L.ed25519_SignMessage_multi(h, s1.ctypes.data, priv.ctypes.data, msg.ctypes.data, 32, n), "sign multi (2^20 + 5)")
        assert sha(s1[: 1 << 20]) == DIG[str(1 << 20)]["ed25519_sig"]
        assert np.array_equal(s1[1 << 20:], api.ed25519_SignMessage(priv[1 << 20:], msg[1 << 20:]))
        vsig, vmsg, bad = synth.corrupt_for_verify(s1, msg)
        ok = np.full(n, -1, np.int32)
        _lib.check(L.ed25519_VerifySignature_multi(h, ok.ctypes.data, vsig.ctypes.data, pub.ctypes.data, vmsg.ctypes.data, 32, n), "verify multi (2^20 + 5)")
        assert np.array_equal(ok == 0, bad) and set(np.unique(ok)) <= {0, 1}
        assert sha(ok[: 1 << 20].astype("<i4")) == DIG[str(1 << 20)]["ed25519_verdicts"]
    finally:
        L.c25519_amd_multi_destroy(h)
    # the environment's way to the same handle: C25519_AMD_MULTI_VIRTUAL (tunable MULTI_VIRTUAL) with a one-device list
    with _lib.tunable("MULTI_VIRTUAL", 3):
        one = (C.c_int * 1)(0)
        _lib.check(L.c25519_amd_multi_create(C.byref(h), one, 1), "c25519_amd_multi_create (MULTI_VIRTUAL=3)")
        try:
            assert L.c25519_amd_multi_device_count(h) == 3
            n = 1000
            sk, pk = R1024["x_sk"][:n].copy(), np.ascontiguousarray(R1024["x_pk"][:n])
            shared = np.empty((n, 32), np.uint8)
            _lib.check(L.curve25519_dh_CreateSharedKey_multi(h, shared.ctypes.data, pk.ctypes.data, sk.ctypes.data, n), "x25519 multi (3 virtual)")
            assert np.array_equal(shared, R1024["x_shared"][:n])
        finally:
            L.c25519_amd_multi_destroy(h)


def test_host_api_soak_with_every_layer_in_the_mix():
    """tools/stress_host_api.py: eight host threads at once, each hammering the *_batch calls (every shape of the pipeline:
    zero-copy calls of a few rows, per-wave kernels, one piece, eight pieces, ragged tails, page-locked and pageable arguments),
    blinded signatures, one-key two-phase verification (per-wave, reference-order and wide-comb kernels with the thread's
    remembered key comb) and its own *_multi handle of three virtual devices in either gather mode -- every result compared
    with the bytes of the plain calls.  This is the run that caught fills of freshly grown result buffers landing AFTER the
    kernels' results on a busy device (hipMemset on the null stream against non-blocking streams: capi_common.hpp,
    zero_device_now)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stress_host_api.py"), "--threads", "8", "--iters", "240"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "stress ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_two_multi_handles_in_two_threads_share_the_copy_threads(api):
    """Two *_multi handles (three and two virtual devices) driven from two host threads at the same time: five pipelines, two
    gathers and two hand-overs feed ONE process-wide pool of copy threads (host_pipeline.hpp: SharedCopyPool) -- every call
    still gets its own bytes (the fixture's, i.e. the reference's), whichever thread's chunks the pool serves first."""
    import threading
    from curve25519_amd import _lib
    L = _lib.load()
    n = (1 << 17) + 3
    sk, pk = synth.x25519_inputs(n)
    esk, msg = synth.ed25519_inputs(n)
    pub, priv = api.ed25519_CreateKeyPair(esk)
    exp_shared, exp_sk = api.curve25519_dh_CreateSharedKey(pk, sk)
    exp_sig = api.ed25519_SignMessage(priv, msg)
    errors = []

    def run(D, which):
        try:
            h = C.c_void_p()
            _lib.check(L.c25519_amd_multi_create(C.byref(h), (C.c_int * D)(*([0] * D)), D), "create")
            try:
                for rep in range(3):
                    if which == "x25519":
                        out, s2 = np.zeros((n, 32), np.uint8), sk.copy()
                        _lib.check(L.curve25519_dh_CreateSharedKey_multi(h, out.ctypes.data, pk.ctypes.data, s2.ctypes.data, n), "x25519 multi")
                        assert np.array_equal(out, exp_shared) and np.array_equal(s2, exp_sk), (D, rep)
                    else:
                        out = np.zeros((n, 64), np.uint8)
                        _lib.check(L.ed25519_SignMessage_multi(h, out.ctypes.data, priv.ctypes.data, msg.ctypes.data, 32, n), "sign multi")
                        assert np.array_equal(out, exp_sig), (D, rep)
            finally:
                L.c25519_amd_multi_destroy(h)
        except BaseException as e:            # noqa: B902 -- carried to the main thread
            errors.append(repr(e))

    ts = [threading.Thread(target=run, args=(3, "x25519")), threading.Thread(target=run, args=(2, "sign"))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=240)
    assert not errors and not any(t.is_alive() for t in ts), errors


def test_host_pointer_api_keeps_up_with_the_device_rate(api):
    """The *_batch entry point a C caller of the drop-in API uses (pageable host arrays in and out) must stay close to
    the device-resident rate at the benchmark size: pinned staging, two stage-in threads and one stage-out thread keep
    both PCIe directions under the kernels.  Measured 0.83 on MI355X (profiles/r02_hostapi.txt); round 1 was 0.48."""
    import time
    import torch
    from curve25519_amd import _lib
    L = _lib.load()
    n = 1 << 20
    sk, pk = synth.x25519_inputs(n)
    out = np.zeros((n, 32), np.uint8)
    dev = torch.device("cuda", 0)
    dsk, dpk, dout = torch.from_numpy(sk).to(dev), torch.from_numpy(pk).to(dev), torch.empty((n, 32), dtype=torch.uint8, device=dev)

    def host():
        assert L.curve25519_dh_CreateSharedKey_batch(out.ctypes.data, pk.ctypes.data, sk.ctypes.data, n) == 0

    def device():
        api.curve25519_dh_CreateSharedKey_dev(dout, dpk, dsk)
        torch.cuda.synchronize()

    best = {}
    for name, fn in (("host", host), ("dev", device)):
        fn()
        fn()
        ts = []
        for _ in range(10):                    # best of ten: the boxes' host cores are shared with other tenants
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        best[name] = min(ts)
    assert np.array_equal(out, dout.cpu().numpy())
    ratio = best["dev"] / best["host"]
    print(f"host-pointer X25519: {n / best['host'] / 1e6:.1f} M ops/s, device-resident {n / best['dev'] / 1e6:.1f} M ops/s, ratio {ratio:.2f}")
    # measured 0.85-0.90 (round 1: 0.48); the bar leaves room for a busy host: the staging copies run on cores this box
    # shares with other tenants, and the device side got faster in round 4 (8.5 ms) while the host side did not
    assert ratio >= 0.72, best


@pytest.mark.parametrize("ranks,batch", [(2, 1 << 16), (8, 1 << 14)])
def test_bench_self_launches_two_ranks(ranks, batch):
    """`python bench.py --gpus N` exactly as the driver invokes it, on a box with ONE GPU: C25519_BENCH_SHARE_GPU lets the
    N ranks share it (gloo gather, since RCCL refuses a duplicate device), so the self-launch under
    torch.distributed.run, the rank / seed / gather bookkeeping and the single JSON line from rank 0 are exercised
    for real -- with 2 ranks and with the 8 of the node the scaling bench runs on.  (The RCCL gather itself runs in
    --dist-selftest with a world of one.)  Every rank is a process that holds its device open, and a shared device takes
    at most SHARED_GPU_MAX_PROCESSES of them, this test's own included: more ranks than that need more GPUs."""
    import torch
    have = torch.cuda.device_count()
    if have < ranks and 1 + ranks > SHARED_GPU_MAX_PROCESSES:
        pytest.skip(f"needs {ranks} GPUs, found {have} ({ranks} ranks sharing them would be more than "
                    f"{SHARED_GPU_MAX_PROCESSES} processes on one GPU)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    if have < ranks:
        env["C25519_BENCH_SHARE_GPU"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "2", "--warmup", "1",
                        "--batch", str(batch), "--no-cpu"], capture_output=True, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(p.stdout.strip().splitlines()) == 1, p.stdout
    line = json.loads(p.stdout)
    assert line["n_gpus"] == ranks and line["config"]["global_batch"] == ranks * batch and line["value"] > 0
    assert sorted(r["rank"] for r in line["per_rank"]) == list(range(ranks))
    assert all(r["kernel_ms"] > 0 and r["step_ms"] > 0 for r in line["per_rank"])
    assert line["verify"]["n_gpus"] == ranks and line["verify"]["rejects_exactly_the_corrupted"] is True
    assert len(line["verify"]["per_rank"]) == ranks
    # every rank hashed its own last output buffers of every pass against the reference's digest for ITS seeded inputs
    for name in ("x25519", "verify", "sign"):
        assert line["bit_exact"][name] == [True] * ranks, (name, line["bit_exact"])
    assert line["bit_exact"]["all"] is True
    assert all(r["bit_exact"] is True and r["ramp_launches"] >= 1 for r in line["per_rank"])
    assert len(line["per_rank_shader_clock_GHz"]) == ranks and all(1.0 < c < 3.0 for c in line["per_rank_shader_clock_GHz"])


def test_bench_dump_outputs_are_what_the_timed_path_computed(tmp_path, oracle):
    """bench.py --dump-outputs DIR writes the last timed step's outputs: the mixed workload at 2^18 (thirds of more than 2^16
    rows: seeded samples) and the default workload's X25519 block at 2^14 (every row), checked against the oracle on the
    same seeded inputs; verdicts reject exactly the corrupted entries."""
    def run(out, extra, n):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu",
                            "--batch", str(n), "--dump-outputs", str(out)] + extra, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads(p.stdout)
        assert line["dump_outputs"]["dir"] == str(out) and line["bit_exact"]["mismatch"] is False
        files = sorted(os.listdir(out))
        assert sorted(line["dump_outputs"]["files"]) == files
        assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
        return files

    def load(out, name, m):
        a = np.load(out / (name + ".npy"))
        rows = np.load(out / (name + "_rows.npy")).astype(np.int64) if os.path.exists(out / (name + "_rows.npy")) else np.arange(m)
        assert a.shape[0] == rows.shape[0] and np.all(np.diff(rows) > 0) and rows[-1] < m
        return a.astype(np.int64), rows

    n = 1 << 18
    files = run(tmp_path / "mixed", ["--workload", "mixed"], n)
    assert files == sorted(f"mixed_{k}{r}.npy" for k in ("x25519_shared", "x25519_sk_clamped", "sign_signatures", "verify_verdicts")
                           for r in ("", "_rows"))
    out = tmp_path / "mixed"
    (x0, x1), (s0, s1), (v0, v1) = synth.mixed_thirds(n)
    sk, pk = synth.x25519_inputs(n)
    got, rows = load(out, "mixed_x25519_shared", x1 - x0)
    got_sk, rows_sk = load(out, "mixed_x25519_sk_clamped", x1 - x0)
    assert np.array_equal(rows, rows_sk)
    few = rows[:1024] + x0
    exp, exp_sk = oracle.x25519_shared(pk[few], sk[few], threads=8)
    assert np.array_equal(got[:1024], exp) and np.array_equal(got_sk[:1024], exp_sk)
    esk, msg = synth.ed25519_inputs(n)
    got, rows = load(out, "mixed_sign_signatures", s1 - s0)
    few = rows[:1024] + s0
    _, priv = oracle.ed25519_keypair(esk[few], threads=8)
    assert np.array_equal(got[:1024], oracle.ed25519_sign(priv, msg[few], threads=8))
    got, rows = load(out, "mixed_verify_verdicts", v1 - v0)
    _, _, bad = synth.corrupt_for_verify(np.zeros((n, 64), np.uint8), np.zeros((n, 32), np.uint8))
    assert np.array_equal(got.reshape(-1) == 0, bad[v0:v1][rows])

    n = 1 << 14
    assert run(tmp_path / "x", ["--no-side"], n) == sorted(["x25519_shared.npy", "x25519_sk_clamped.npy"])
    sk, pk = synth.x25519_inputs(n)
    exp, exp_sk = oracle.x25519_shared(pk, sk, threads=8)
    assert np.array_equal(load(tmp_path / "x", "x25519_shared", n)[0], exp)
    assert np.array_equal(load(tmp_path / "x", "x25519_sk_clamped", n)[0], exp_sk)


def test_bench_detects_a_wrong_output_and_exits_nonzero():
    """The bit_exact check has teeth: with the digests file pointing at other expectations (rank 1's digests where rank 0's
    belong) the line says mismatch and the process exits non-zero."""
    import tempfile
    with open(os.path.join(GOLD, "digests.json")) as f:
        d = json.load(f)
    d["ranks"]["by_rank"][0], d["ranks"]["by_rank"][1] = d["ranks"]["by_rank"][1], d["ranks"]["by_rank"][0]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "digests.json")
        with open(path, "w") as f:
            json.dump(d, f)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--no-cpu", "--no-side",
                            "--batch", str(1 << 14)], capture_output=True, text=True, timeout=240,
                           env={**os.environ, "C25519_BENCH_DIGESTS": path})
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])
    line = json.loads(p.stdout)
    assert line["bit_exact"]["x25519"] is False and line["bit_exact"]["mismatch"] is True and line["bit_exact"]["all"] is False


def test_a_late_rank_does_not_change_the_timed_region():
    """bench.py's protocol: the clock-ramp launches come BEHIND the opening barrier, directly in front of the timed steps, and
    a rank's time is its own t1 - t0 -- so a rank that arrives half a second late at every block (C25519_BENCH_DELAY_RANK0_S;
    round 4's live probe on rank 0 was such a delay, in front of the side blocks) starts its timed steps on a chip that has
    just been busy for 60 ms, not on the clock ramp (10-19 % slow, profiles/r04_warmup_probe.txt).  The N > 1 code path with
    a world of one rank (RCCL gathers), 2^20 per pass; sign is the pass most sensitive to the ramp (1.6 ms per step)."""
    res = {}
    for delay in ("0", "0.5"):
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
        env["C25519_BENCH_DELAY_RANK0_S"] = delay
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dist-selftest", "--steps", "20", "--warmup", "2",
                            "--no-cpu"], capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        res[delay] = json.loads(p.stdout)
        assert res[delay]["bit_exact"]["all"] is True
    for name in ("x25519", "verify", "sign"):
        a = res["0"]["ms_per_step"] if name == "x25519" else res["0"][name]["ms_per_step"]
        b = res["0.5"]["ms_per_step"] if name == "x25519" else res["0.5"][name]["ms_per_step"]
        # (run-to-run noise of a 20-step block is ~2 %; timed on the ramp X25519 reads 11 %, verification 10 %, signing 19 % slow)
        assert abs(a - b) / a < (0.08 if name == "sign" else 0.06), (name, a, b)


def test_small_calls_run_one_operation_per_wave_and_agree_with_the_batch_kernels(api, oracle, monkeypatch):
    """Calls of a few elements -- the reference's own single-call prototypes are calls of one -- run ONE operation per wave
    (csrc/coop25519.cuh: a field element limb-per-lane, four products at a time; 4-5 x less latency), larger ones one
    operation per lane.  Both shapes against the oracle and against each other around the switch, for every operation
    that has both (the tunable COOP_MAX: 0 forces the batch kernels, a large value the per-wave ones)."""
    import vectors
    for n in (1, 2, 63, 64, 65, 300):
        sk, pk = synth.random_bytes((n, 32), 0x7001 + n), synth.random_bytes((n, 32), 0x7101 + n)
        sk[0], pk[0] = 0xff, 0xff                                     # all-ones key and peer (bit 255 set, >= p)
        if n > 2:
            pk[1] = vectors.le(2**255 - 19, 32)                       # p itself: a zero point, zero bytes out
            pk[2] = 0                                                 # low order
        esk, msg = synth.random_bytes((n, 32), 0x7201 + n), synth.random_bytes((n, 37), 0x7301 + n)
        got = {}
        from curve25519_amd import _lib
        for mode, knob in (("per wave", 1 << 20), ("per lane", 0)):
            _lib.set_tunable("COOP_MAX", knob)
            shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
            base, _ = api.curve25519_dh_CalculatePublicKey(sk)
            fast, _ = api.curve25519_dh_CalculatePublicKey(sk, fast=True)
            pub, priv = api.ed25519_CreateKeyPair(esk)
            sig = api.ed25519_SignMessage(priv, msg)
            got[mode] = (shared, clamped, base, fast, pub, priv, sig)
        _lib.set_tunable("COOP_MAX", -1)
        for a, b in zip(got["per wave"], got["per lane"]):
            assert np.array_equal(a, b), n
        shared, clamped, base, fast, pub, priv, sig = got["per wave"]
        exp_shared, exp_clamped = oracle.x25519_shared(pk, sk)
        assert np.array_equal(shared, exp_shared) and np.array_equal(clamped, exp_clamped)
        assert np.array_equal(base, fast) and np.array_equal(base, oracle.x25519_shared(np.tile(vectors.le(9, 32), (n, 1)), sk)[0])
        epub, epriv = oracle.ed25519_keypair(esk)
        assert np.array_equal(pub, epub) and np.array_equal(priv, epriv) and np.array_equal(sig, oracle.ed25519_sign(epriv, msg))
    # messages of other lengths through the per-wave signing kernel (the hashing is the batch kernels' code, run by every lane)
    for mlen in (0, 1, 111, 112, 200):
        esk, msg = synth.random_bytes((5, 32), 0x7401 + mlen), synth.random_bytes((5, mlen), 0x7501 + mlen)
        pub, priv = api.ed25519_CreateKeyPair(esk)
        assert np.array_equal(api.ed25519_SignMessage(priv, msg), oracle.ed25519_sign(priv, msg))


def test_x25519_calls_of_a_few_elements_run_the_ladder_on_two_waves(api, oracle):
    """curve25519_dh_CreateSharedKey for up to 512 elements per call runs k_x25519_coop2: two waves per element, a ladder step in
    two product levels (one wave the differential addition with x1 times the sum carried along, the other the doubling), operands
    exchanged through LDS behind one workgroup barrier per step.  KATs with every edge public key, fixture rows at 1 / 2 / 511 /
    512 / 513 elements (the last one back on the one-wave kernel) and a random batch, against the reference's bytes and -- tunable
    LADDER2_MAX = 0 / large -- against the one-wave kernel; the clamped secret is written back."""
    from curve25519_amd import _lib
    recs = KAT["x25519"]
    pk, sk = np.concatenate([h2a(r["pk"]) for r in recs]), np.concatenate([h2a(r["sk"]) for r in recs])
    shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
    for i, r in enumerate(recs):
        assert shared[i].tobytes().hex() == r["shared"] and clamped[i].tobytes().hex() == r["sk_clamped"], r["name"]
    g = R1024
    for n in (1, 2, 511, 512, 513, 1000):
        got = {}
        for knob in (0, 1 << 20):
            with _lib.tunable("LADDER2_MAX", knob):
                got[knob] = api.curve25519_dh_CreateSharedKey(g["x_pk"][:n], g["x_sk"][:n])
        default = api.curve25519_dh_CreateSharedKey(g["x_pk"][:n], g["x_sk"][:n])
        for shared, clamped in (got[0], got[1 << 20], default):
            assert np.array_equal(shared, g["x_shared"][:n]) and np.array_equal(clamped, g["x_sk_clamped"][:n]), n
    n = 700
    sk, pk = synth.random_bytes((n, 32), 0x8801), synth.random_bytes((n, 32), 0x8802)
    pk[3], pk[4] = 0, 255                                              # a low-order point; 2^256 - 1
    with _lib.tunable("LADDER2_MAX", 1 << 20):
        shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
    e_shared, e_clamped = oracle.x25519_shared(pk, sk)
    assert np.array_equal(shared, e_shared) and np.array_equal(clamped, e_clamped)


def test_warm_device_calls_can_be_captured_into_a_hip_graph(api, oracle):
    """A *_dev call on a stream that has run it before allocates nothing and synchronises nothing: kernel launches and one
    event record, so a caller may capture it into a HIP graph and replay it.  (Replaying saves nothing -- back-to-back calls
    already keep the queue full: 180 against 181 us for 2^14 signatures, profiles/r04_hip_graph.txt -- but it must work.)"""
    import torch
    dev = torch.device("cuda", 0)
    n = 5000
    esk, msg = synth.random_bytes((n, 32), 0x7801), synth.random_bytes((n, 40), 0x7802)
    pub_h, priv_h = api.ed25519_CreateKeyPair(esk)
    exp_sig = oracle.ed25519_sign(priv_h, msg)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    priv, msgd, pub = up(priv_h), up(msg), up(pub_h)
    sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    ok = torch.empty((n, 1), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)

    def step():
        api.ed25519_SignMessage_dev(sig, priv, msgd)
        api.ed25519_VerifySignature_dev(ok, sig, pub, msgd)

    with torch.cuda.stream(s):
        step()                                                      # warm: the stream's work scratch exists now
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    for _ in range(3):
        sig.zero_(); ok.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(sig.cpu().numpy(), exp_sig) and bool(ok.all().item())


def test_degenerate_but_valid_signatures_on_both_paths(api):
    """tests/golden/degenerate_verify.npz through ed25519_VerifySignature on the device: the default pass (lattice path +
    slow list) with BOTH shapes forced explicitly -- k_ed25519_verify_one_per_group (one element per two-wave workgroup: tunable
    COOP_MAX large) and k_ed25519_verify_fast_walk (one per lane: COOP_MAX 0) -- and with VERIFY_REFERENCE_ORDER = 1 (every
    element through the reference-order kernels).  Expected verdicts are the real reference's: 336 of these 1024
    signatures over small-order / mixed-order keys, small-order R in every encoding and S in {0, L, 2L, 15L} are VALID
    for it (ed25519_verify.c:287-313 has no S < L and no small-order check)."""
    from curve25519_amd import _lib
    L = _lib.load()
    d = np.load(os.path.join(GOLD, "degenerate_verify.npz"))
    sig, pk, msg, exp = (np.ascontiguousarray(d[k]) for k in ("sig", "pk", "msg", "verdict"))
    assert np.array_equal(api.ed25519_VerifySignature(sig, pk, msg), exp)
    for knob in (1 << 20, 0):                                         # per wave, per lane
        with _lib.tunable("COOP_MAX", knob):
            assert np.array_equal(api.ed25519_VerifySignature(sig, pk, msg), exp), knob
            assert L.c25519_amd_verify_last_slow_elements() >= 0      # the lattice path ran (some of these keys are off the curve)
    # inside a big batch of ordinary signatures too (other workgroup shapes, sorted walk order)
    n = 1 << 14
    sk, m8 = synth.random_bytes((n, 32), 0x411), synth.random_bytes((n, 8), 0x422)
    pub, priv = api.ed25519_CreateKeyPair(sk)
    s2 = api.ed25519_SignMessage(priv, m8)
    at = np.arange(len(exp)) * 13 + 5
    s2[at], pub[at], m8[at] = sig, pk, msg
    want = np.ones(n, np.int32)
    want[at] = exp
    assert np.array_equal(api.ed25519_VerifySignature(s2, pub, m8), want)
    with _lib.tunable("VERIFY_REFERENCE_ORDER", 1):
        assert np.array_equal(api.ed25519_VerifySignature(sig, pk, msg), exp)
        assert L.c25519_amd_verify_last_slow_elements() == -1         # no lattice path in that call
        assert np.array_equal(api.ed25519_VerifySignature(s2, pub, m8), want)


def test_overlong_lattice_vectors_take_the_reference_order_path(api, oracle):
    """The walk of the lattice path takes short vectors up to LAT_CAP_BITS = 158 bits (verify_fast.cuh); a longer one -- 2^-33
    per random h -- sends its element to the slow list and k_ed25519_verify_slow decides it in the reference's order
    (ed25519_verify.c:287-313).  The test knob VERIFY_LAT_CAP_BITS lowers the cap INTO the typical range (127-131 bits), so
    that about half of a batch of ordinary signatures takes that branch on the device -- on-curve keys on the slow list,
    which garbage keys never exercise -- mixed with the corrupted entries and S + L: verdicts against the oracle, the
    accounting hook counts the detour, and the same inputs under the production cap take no detour at all."""
    from curve25519_amd import _lib
    import vectors
    L = _lib.load()
    n = 1 << 14
    sk, msg = synth.random_bytes((n, 32), 0x6a1), synth.random_bytes((n, 21), 0x6a2)
    pub, priv = api.ed25519_CreateKeyPair(sk)
    sig = api.ed25519_SignMessage(priv, msg)
    bsig, bmsg, bad = synth.corrupt_for_verify(sig, msg)
    for i in range(0, 300, 3):                                           # S + L: accepted by the reference
        S = int.from_bytes(bsig[i, 32:].tobytes(), "little")
        if S + vectors.L < 2**256:
            bsig[i, 32:] = vectors.le(S + vectors.L, 32)
    exp = oracle.ed25519_verify(bsig, pub, bmsg, threads=THREADS)
    assert np.array_equal(exp == 0, bad)
    seen = []
    for cap in (128, 126, 131):
        with _lib.tunable("VERIFY_LAT_CAP_BITS", cap):
            for knob in (-1, 0):                                         # both walk kernels around the slow list
                with _lib.tunable("COOP_MAX", knob):
                    ok = api.ed25519_VerifySignature(bsig, pub, bmsg)
                    slow = L.c25519_amd_verify_last_slow_elements()
                    assert np.array_equal(ok, exp), (cap, knob)
            seen.append(slow)
    assert n // 8 < seen[0] < n - n // 8 and seen[1] > seen[0] > seen[2] > 0, seen    # roughly half at 128 bits, monotone in the cap
    # a few elements only (the per-wave kernels' shapes) with the cap lowered
    with _lib.tunable("VERIFY_LAT_CAP_BITS", 127):
        for m in (1, 5, 64):
            assert np.array_equal(api.ed25519_VerifySignature(bsig[:m], pub[:m], bmsg[:m]), exp[:m]), m
    ok = api.ed25519_VerifySignature(bsig, pub, bmsg)
    assert L.c25519_amd_verify_last_slow_elements() == 0 and np.array_equal(ok, exp)


def test_lattice_fast_path_and_reference_order_agree(api, oracle):
    """ed25519_VerifySignature's default path decides every element whose key is on the curve with the exact lattice-shortened walk
    (csrc/verify_fast.cuh) and runs the reference's operation order for the rest.  Every class of input where the two
    could differ, against the oracle: corrupted signatures, S >= L, keys / R's with torsion components (a cofactored
    check would accept eight times as many), small-order keys, R encodings no encoder produces, garbage.  The
    accounting hook shows which path really ran."""
    from curve25519_amd import _lib
    import vectors
    L = _lib.load()
    n = 1 << 14
    sk, msg = synth.random_bytes((n, 32), 0x111), synth.random_bytes((n, 40), 0x222)
    pub, priv = api.ed25519_CreateKeyPair(sk)
    sig = api.ed25519_SignMessage(priv, msg)
    bsig, bmsg, bad = synth.corrupt_for_verify(sig, msg)
    for i in range(0, 600, 3):                                           # S + L: accepted by the reference
        S = int.from_bytes(bsig[i, 32:].tobytes(), "little")
        if S + vectors.L < 2**256:
            bsig[i, 32:] = vectors.le(S + vectors.L, 32)
    ok = api.ed25519_VerifySignature(bsig, pub, bmsg)
    assert L.c25519_amd_verify_last_slow_elements() == 0                  # all keys on the curve: the fast path took everything
    assert np.array_equal(ok, oracle.ed25519_verify(bsig, pub, bmsg, threads=THREADS)) and np.array_equal(ok == 0, bad)
    # torsion, small order, special R
    tsig, tpk, tmsg = vectors.torsion_signature_cases(count=40)
    ok = api.ed25519_VerifySignature(tsig, tpk, tmsg)
    exp = oracle.ed25519_verify(tsig, tpk, tmsg)
    assert np.array_equal(ok, exp) and 0 < exp.sum() < len(exp) // 4 and L.c25519_amd_verify_last_slow_elements() == 0
    lo = vectors.small_order_keys()
    gs, gm = synth.random_bytes((8, 64), 41), synth.random_bytes((8, 32), 42)
    assert np.array_equal(api.ed25519_VerifySignature(gs, lo, gm), oracle.ed25519_verify(gs, lo, gm))
    sp = vectors.special_r_encodings()
    m = sp.shape[0]
    ssig = np.ascontiguousarray(np.concatenate([sp, bsig[:m, 32:]], axis=1))
    assert np.array_equal(api.ed25519_VerifySignature(ssig, pub[:m], bmsg[:m]), oracle.ed25519_verify(ssig, pub[:m], bmsg[:m]))
    # a garbage key in a batch sends exactly its own element down the reference-order path (the slow list)
    mixed = pub.copy()
    gkey = synth.random_bytes((64, 32), 0x999)
    off = next(k for k in gkey if vectors.ed_decode(int.from_bytes(k.tobytes(), "little") & (2**255 - 1), 0) is None)
    mixed[1000], mixed[9000] = off, off
    ok = api.ed25519_VerifySignature(bsig, mixed, bmsg)
    assert L.c25519_amd_verify_last_slow_elements() == 2
    assert np.array_equal(ok, oracle.ed25519_verify(bsig, mixed, bmsg, threads=THREADS))
    # the same inputs with the fast path switched off give the same verdicts
    with _lib.tunable("VERIFY_REFERENCE_ORDER", 1):
        ref_order = api.ed25519_VerifySignature(bsig, mixed, bmsg)
        assert L.c25519_amd_verify_last_slow_elements() == -1
    assert np.array_equal(ref_order, ok)


@pytest.mark.parametrize("knobs", [{"C25519_AMD_BATCH_PIECES": "24", "C25519_AMD_STAGERS": "3", "C25519_AMD_DRAINERS": "2"},
                                   {"C25519_AMD_BATCH_PIECES": "2", "C25519_AMD_STAGERS": "1", "C25519_AMD_DRAINERS": "1"}])
def test_host_pipeline_shapes_give_the_same_bytes(api, oracle, knobs):
    """The *_batch pipeline (engine.hip run_batch) in shapes the default call never takes: more pieces than buffer
    sets (a set is reused only after its previous piece was copied out), several stage-in / stage-out threads, and the
    two-piece minimum.  Same bytes as the default shape, and a sample of them against the oracle."""
    n = 300001
    sk, pk = synth.x25519_inputs(n)
    esk, msg = synth.ed25519_inputs(n)
    shared, _ = api.curve25519_dh_CreateSharedKey(pk, sk)
    pub, priv = api.ed25519_CreateKeyPair(esk)
    sig = api.ed25519_SignMessage(priv, msg)
    bsig, bmsg, bad = synth.corrupt_for_verify(sig, msg)
    ok = api.ed25519_VerifySignature(bsig, pub, bmsg)
    assert np.array_equal(ok == 0, bad)
    idx = np.arange(0, n, 997)
    assert np.array_equal(shared[idx], oracle.x25519_shared(np.ascontiguousarray(pk[idx]), np.ascontiguousarray(sk[idx]))[0])
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r)\n"
        "from curve25519_amd import api\n"
        "d = np.load(sys.argv[1])\n"
        "shared, _ = api.curve25519_dh_CreateSharedKey(d['pk'], d['sk'])\n"
        "pub, priv = api.ed25519_CreateKeyPair(d['esk'])\n"
        "sig = api.ed25519_SignMessage(priv, d['msg'])\n"
        "ok = api.ed25519_VerifySignature(d['bsig'], pub, d['bmsg'])\n"
        "np.savez(sys.argv[2], shared=shared, pub=pub, priv=priv, sig=sig, ok=ok)\n") % ROOT
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), pk=pk, sk=sk, esk=esk, msg=msg, bsig=bsig, bmsg=bmsg)
        p = subprocess.run([sys.executable, "-c", code, os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")],
                           capture_output=True, text=True, timeout=300, env={**os.environ, **knobs})
        assert p.returncode == 0, p.stderr[-2000:]
        out = np.load(os.path.join(tmp, "out.npz"))
        for name, want in (("shared", shared), ("pub", pub), ("priv", priv), ("sig", sig), ("ok", ok)):
            assert np.array_equal(out[name], want), name


def test_page_locked_caller_arrays_are_used_in_place(api, oracle):
    """*_batch recognises page-locked arguments (c25519_amd_host_register on page-aligned buffers, or hipHostMalloc
    memory such as torch's pinned tensors) and lets the copy engines work on them directly; any mix of locked and
    pageable arguments, the IN/OUT secret-key array included, gives the bytes of the ordinary call."""
    import torch
    from curve25519_amd import _lib
    L = _lib.load()
    n = 200003
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    sk, pk = synth.x25519_inputs(n)
    want, want_sk = api.curve25519_dh_CreateSharedKey(pk, sk)
    # every argument registered (buffers in pages of their own: the call refuses anything else)
    r_sk, r_pk, r_out = synth.page_aligned((n, 32), like=sk), synth.page_aligned((n, 32), like=pk), synth.page_aligned((n, 32))
    for a in (r_sk, r_pk, r_out):
        assert L.c25519_amd_host_register(P(a), synth.locked_bytes(a)) == 0
    assert L.curve25519_dh_CreateSharedKey_batch(P(r_out), P(r_pk), P(r_sk), n) == 0
    assert np.array_equal(r_out, want) and np.array_equal(r_sk, want_sk), "clamped in place, in the caller's locked array"
    # only the output registered, inputs pageable; then only one input
    p_sk = sk.copy()
    r_out[:] = 0
    assert L.curve25519_dh_CreateSharedKey_batch(P(r_out), P(pk), P(p_sk), n) == 0
    assert np.array_equal(r_out, want) and np.array_equal(p_sk, want_sk)
    out = np.zeros((n, 32), np.uint8)
    p_sk = sk.copy()
    assert L.curve25519_dh_CreateSharedKey_batch(P(out), P(r_pk), P(p_sk), n) == 0
    assert np.array_equal(out, want)
    # a window into a registered array that ends at its last byte, and one that starts inside it
    m = 70001
    out = np.zeros((m, 32), np.uint8)
    t_sk = r_sk[n - m:].copy()
    assert L.c25519_amd_host_register(P(r_sk[1:]), 4096) != 0 and b"whole pages" in L.c25519_amd_last_error()
    assert L.curve25519_dh_CreateSharedKey_batch(P(out), P(r_pk[n - m:]), P(t_sk), m) == 0
    assert np.array_equal(out, want[n - m:])
    for a in (r_sk, r_pk, r_out):
        assert L.c25519_amd_host_unregister(P(a)) == 0
    # torch's pinned tensors (hipHostMalloc) through sign + verify
    esk, msg = synth.ed25519_inputs(n)
    pub, priv = api.ed25519_CreateKeyPair(esk)
    sig = api.ed25519_SignMessage(priv, msg)
    pin = {k: torch.from_numpy(v).pin_memory() for k, v in dict(priv=priv, msg=msg, pub=pub).items()}
    t_sig = torch.zeros((n, 64), dtype=torch.uint8).pin_memory()
    t_ok = torch.zeros(n, dtype=torch.int32).pin_memory()
    D = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.ed25519_SignMessage_batch(D(t_sig), D(pin["priv"]), D(pin["msg"]), msg.shape[1], n) == 0
    assert np.array_equal(t_sig.numpy(), sig)
    bsig, bmsg, bad = synth.corrupt_for_verify(sig, msg)
    t_sig.copy_(torch.from_numpy(bsig))
    assert L.ed25519_VerifySignature_batch(D(t_ok), D(t_sig), D(pin["pub"]), P(bmsg), bmsg.shape[1], n) == 0
    assert np.array_equal(t_ok.numpy() == 0, bad)


def test_x25519_on_four_lanes_per_element(api, oracle):
    """k_x25519_quad (quad25519.cuh): a quad of lanes per element, one product of the ladder step per lane and level, operands
    exchanged with v_mov_b32_dpp quad_perm -- what calls of 2^12 .. 2^14 elements run.  Forced (QUAD_MIN = 0) for the KATs with
    every edge public key (zero Z -> zero bytes), the base-point ladder of curve25519_dh_CalculatePublicKey (level 3 is a
    multiplication by 9), fixture rows at 1 / 15 / 16 / 17 / 1000 elements (a lone quad, a wave short of one quad, exactly one
    wave, one quad into the next workgroup), output aliasing the public keys, and at its own sizes by default -- 4609, 5000 and
    2^14 elements -- against the oracle and against the one-lane kernels (QUAD_MAX = 0); the clamped secret is written back."""
    import torch
    import vectors
    from curve25519_amd import _lib
    recs = KAT["x25519"]
    pk, sk = np.concatenate([h2a(r["pk"]) for r in recs]), np.concatenate([h2a(r["sk"]) for r in recs])
    with _lib.tunable("QUAD_MIN", 0), _lib.tunable("QUAD_MAX", 1 << 20):
        shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
        for i, r in enumerate(recs):
            assert shared[i].tobytes().hex() == r["shared"] and clamped[i].tobytes().hex() == r["sk_clamped"], r["name"]
        recs = KAT["x25519_public"]
        pub, clamped = api.curve25519_dh_CalculatePublicKey(np.concatenate([h2a(r["sk"]) for r in recs]))
        for i, r in enumerate(recs):
            assert pub[i].tobytes().hex() == r["pk"] and clamped[i].tobytes().hex() == r["sk_clamped"], r["name"]
        g = R1024
        for n in (1, 15, 16, 17, 1000):
            shared, clamped = api.curve25519_dh_CreateSharedKey(g["x_pk"][:n], g["x_sk"][:n])
            assert np.array_equal(shared, g["x_shared"][:n]) and np.array_equal(clamped, g["x_sk_clamped"][:n]), n
        dev = torch.device("cuda", 0)                                  # `shared` aliasing `pk` (curve25519_dh.c:104,150)
        buf, dsk = torch.from_numpy(g["x_pk"][:333].copy()).to(dev), torch.from_numpy(g["x_sk"][:333].copy()).to(dev)
        api.curve25519_dh_CreateSharedKey_dev(buf, buf, dsk)
        assert np.array_equal(buf.cpu().numpy(), g["x_shared"][:333]) and np.array_equal(dsk.cpu().numpy(), g["x_sk_clamped"][:333])
    for n in (4609, 5000, 1 << 14):                                    # the sizes the dispatch gives to the quads by itself
        sk, pk = synth.random_bytes((n, 32), 0x9901 + n), synth.random_bytes((n, 32), 0x9902 + n)
        pk[3], pk[4], pk[n - 1] = 0, 255, 1                            # a low-order point; 2^256 - 1; another low-order point
        shared, clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
        with _lib.tunable("QUAD_MAX", 0):
            lane_shared, lane_clamped = api.curve25519_dh_CreateSharedKey(pk, sk)
        assert np.array_equal(shared, lane_shared) and np.array_equal(clamped, lane_clamped), n
        if n <= 5000:
            e_shared, e_clamped = oracle.x25519_shared(pk, sk)
            assert np.array_equal(shared, e_shared) and np.array_equal(clamped, e_clamped), n
            pub, _ = api.curve25519_dh_CalculatePublicKey(sk)
            assert np.array_equal(pub, oracle.x25519_shared(np.tile(vectors.le(9, 32), (n, 1)), sk)[0]), n


def test_verification_walk_on_four_lanes_per_element(api, oracle):
    """k_ed25519_verify_quad_walk (quad25519.cuh): the lattice path's walk with a quad of lanes per element -- an addition in two
    product levels (one field of the table row per lane), a doubling as a level of squarings and one of products -- what
    batches of 2^11 .. 2^15 signatures run.  Forced (QUAD_MIN = 0) on the fixture at 1 / 15 / 16 / 17 / 63 / 64 / 65 / 1000
    signatures (a lone quad, wave and workgroup edges) with its rejected entries, on the degenerate vectors (small-order keys and
    R, S >= L, off-curve keys on the slow list: the reference's verdicts), with garbage keys; at its own sizes by default (5000,
    2^14 with corrupted entries) against the oracle and against the one-lane walk (QUAD_MAX = 0)."""
    from curve25519_amd import _lib
    L = _lib.load()
    g = R1024
    with _lib.tunable("QUAD_MIN", 0), _lib.tunable("QUAD_MAX", 1 << 20):
        for n in (1, 15, 16, 17, 63, 64, 65, 1000):
            assert np.array_equal(api.ed25519_VerifySignature(g["v_sig"][:n], g["ed_pub"][:n], g["v_msg"][:n]), g["v_ok"][:n]), n
        d = np.load(os.path.join(GOLD, "degenerate_verify.npz"))
        sig, pk, msg, exp = (np.ascontiguousarray(d[k]) for k in ("sig", "pk", "msg", "verdict"))
        assert np.array_equal(api.ed25519_VerifySignature(sig, pk, msg), exp)
        assert L.c25519_amd_verify_last_slow_elements() >= 0               # the lattice path ran
        n = 700
        mixed = g["ed_pub"][:n].copy()
        mixed[::5] = synth.random_bytes((n, 32), 0x5109)[::5]              # garbage keys: half of them off the curve
        assert np.array_equal(api.ed25519_VerifySignature(g["v_sig"][:n], mixed, g["v_msg"][:n]),
                              oracle.ed25519_verify(g["v_sig"][:n], mixed, g["v_msg"][:n]))
        assert L.c25519_amd_verify_last_slow_elements() > 20               # off-curve keys went to the reference-order kernel
    for n in (5000, 1 << 14):
        sk, msg = synth.random_bytes((n, 32), 0x6b1 + n), synth.random_bytes((n, 33), 0x6b2 + n)
        pub, priv = api.ed25519_CreateKeyPair(sk)
        bsig, bmsg, bad = synth.corrupt_for_verify(api.ed25519_SignMessage(priv, msg), msg)
        ok = api.ed25519_VerifySignature(bsig, pub, bmsg)
        with _lib.tunable("QUAD_MAX", 0):
            lane = api.ed25519_VerifySignature(bsig, pub, bmsg)
        assert np.array_equal(ok, lane) and np.array_equal(ok == 0, bad), n
        if n == 5000:
            assert np.array_equal(ok, oracle.ed25519_verify(bsig, pub, bmsg))


def test_fixed_base_operations_on_four_lanes_per_element(api, oracle):
    """k_ed25519_keypair_quad / k_ed25519_sign_quad / k_x25519_public_fast_quad (quad25519.cuh: the walk over the wide comb with a
    quad of lanes per element, inversion, encoding, the last hash and S in the same launch) -- what calls of 2^11 .. 2^14 elements
    run.  Forced (QUAD_MIN = 0) for the RFC 8032 / reference vectors at every message length, the fixture at 1 / 15 / 16 / 17 / 1000
    elements (a lone quad, a wave short of one quad, exactly one wave, one quad into the next workgroup), ragged messages; at
    their own sizes by default (1025, 5000, 2^14) against the oracle and against the per-wave / one-lane kernels (QUAD_MAX = 0)
    and the LDS comb (BASE_COMB = 0)."""
    from curve25519_amd import _lib
    g = R1024
    with _lib.tunable("QUAD_MIN", 0), _lib.tunable("QUAD_MAX", 1 << 20):
        for r in KAT["ed25519"]:
            msg = np.frombuffer(bytes.fromhex(r["msg"]), np.uint8).reshape(1, -1).copy()
            pub, priv = api.ed25519_CreateKeyPair(h2a(r["sk"]))
            assert pub.tobytes().hex() == r["pk"] and priv.tobytes().hex() == r["priv"], r["name"]
            assert api.ed25519_SignMessage(priv, msg).tobytes().hex() == r["sig"], r["name"]
        recs = KAT["x25519_public"]
        pub, clamped = api.curve25519_dh_CalculatePublicKey(np.concatenate([h2a(r["sk"]) for r in recs]), fast=True)
        for i, r in enumerate(recs):
            assert pub[i].tobytes().hex() == r["pk"] and clamped[i].tobytes().hex() == r["sk_clamped"], r["name"]
        for n in (1, 15, 16, 17, 1000):
            pub, priv = api.ed25519_CreateKeyPair(g["ed_sk"][:n])
            assert np.array_equal(pub, g["ed_pub"][:n]) and np.array_equal(priv, g["ed_priv"][:n]), n
            assert np.array_equal(api.ed25519_SignMessage(priv, g["ed_msg"][:n]), g["ed_sig"][:n]), n
        n = 333                                                        # ragged messages through the same kernel
        msgs = [synth.random_bytes(((i * 7) % 200, 1), 0x7a61 + i).reshape(-1).tobytes() for i in range(n)]
        got = api.ed25519_SignMessage_ragged(g["ed_priv"][:n], msgs)
        for i in range(0, n, 9):
            m = np.frombuffer(msgs[i], np.uint8).reshape(1, -1)
            assert np.array_equal(got[i:i + 1], oracle.ed25519_sign(g["ed_priv"][i:i + 1], m)), i
    for n in (1025, 5000, 1 << 14):                                    # the sizes the dispatch gives to the quads by itself
        sk, msg = synth.random_bytes((n, 32), 0x4f1 + n), synth.random_bytes((n, 45), 0x4f2 + n)
        pub, priv = api.ed25519_CreateKeyPair(sk)
        sig = api.ed25519_SignMessage(priv, msg)
        xpub, xclamped = api.curve25519_dh_CalculatePublicKey(sk, fast=True)
        for knob, val in (("QUAD_MAX", 0), ("BASE_COMB", 0)):
            with _lib.tunable(knob, val):
                lpub, lpriv = api.ed25519_CreateKeyPair(sk)
                lxpub, lxclamped = api.curve25519_dh_CalculatePublicKey(sk, fast=True)
                assert np.array_equal(pub, lpub) and np.array_equal(priv, lpriv), (n, knob)
                assert np.array_equal(sig, api.ed25519_SignMessage(priv, msg)), (n, knob)
                assert np.array_equal(xpub, lxpub) and np.array_equal(xclamped, lxclamped), (n, knob)
        if n <= 5000:
            epub, epriv = oracle.ed25519_keypair(sk)
            assert np.array_equal(pub, epub) and np.array_equal(priv, epriv) and np.array_equal(sig, oracle.ed25519_sign(priv, msg)), n


def test_a_remembered_key_comb_serves_batches_of_any_size(api, oracle):
    """One ed25519_Verify_Init, many ed25519_Verify_Check calls (ed25519_verify.c:282-286): the comb a batch of >= 2^16 pairs builds
    for its key stays with the calling thread, and every later call of more than 1024 pairs whose context is that one walks the
    two wide combs again -- at 2^12 and 2^14 pairs, where building a comb (0.6 ms) would not pay -- while another key's context,
    a tampered copy and a call before any comb exists keep the reference-order kernel.  c25519_amd_verify_check_last_wide says
    which path decided; the verdicts are the oracle's either way."""
    from curve25519_amd import _lib
    L = _lib.load()
    big = 1 << 16
    sk = synth.random_bytes((2, 32), 0x7b03)
    pub, priv = oracle.ed25519_keypair(sk)
    ctx = api.ed25519_Verify_Init(pub)
    msg = synth.random_bytes((big, 19), 0x7b04)
    sig = [oracle.ed25519_sign(np.repeat(priv[k:k + 1], big, axis=0), msg, threads=THREADS) for k in range(2)]
    for s in sig:
        s[5::11, 40] ^= 4                                              # rejected entries in every batch
    want = [oracle.ed25519_verify(sig[k], np.repeat(pub[k:k + 1], big, axis=0), msg, threads=THREADS) for k in range(2)]
    assert 0 < want[0].sum() < big

    def check(k, n, expect_wide, cx=None):
        got = api.ed25519_Verify_Check(ctx[k] if cx is None else cx, sig[k][:n], msg[:n])
        path = L.c25519_amd_verify_check_last_wide()
        assert path == expect_wide, (k, n, path)
        return got

    L.c25519_amd_thread_release()                                      # this thread remembers nothing
    assert np.array_equal(check(0, 1 << 12, 0), want[0][:1 << 12])      # no comb yet: reference order
    assert np.array_equal(check(0, big, 1), want[0])                    # builds and remembers key 0's comb
    for n in (1 << 12, 1 << 14, 5000, 1025):
        assert np.array_equal(check(0, n, 1), want[0][:n]), n           # the remembered comb, at any size
        assert np.array_equal(check(1, n, 0), want[1][:n]), n           # another key: not worth a comb at this size
        assert np.array_equal(check(0, n, 1), want[0][:n]), n           # ... and key 0's comb is still the remembered one
    tampered = ctx[0].copy()
    tampered[32 + 128 * 3 + 9] ^= 0x10
    bent = check(0, 1 << 12, 0, cx=tampered)                            # not the remembered bytes: the rows are read as they are
    with _lib.tunable("ONE_KEY_WIDE", 0):
        assert np.array_equal(bent, api.ed25519_Verify_Check(tampered, sig[0][:1 << 12], msg[:1 << 12]))
        assert np.array_equal(check(0, 1 << 14, 0), want[0][:1 << 14])  # the knob turns the comb path off altogether
    assert np.array_equal(check(0, 1000, 0), want[0][:1000])            # per-wave kernels' range
    assert np.array_equal(check(1, big, 1), want[1])                    # key 1 takes the buffer over ...
    assert np.array_equal(check(0, 1 << 12, 0), want[0][:1 << 12])      # ... and key 0 is no longer remembered
    assert np.array_equal(check(1, 1 << 12, 1), want[1][:1 << 12])


def test_single_calls_with_large_messages_are_uploaded_not_read_over_pcie(api, oracle):
    """A call of a few elements reads its operands straight out of pinned host memory (no copy commands) -- but only while they
    are small: a message of KiB .. MiB is hashed byte by byte (twice when signing), which over PCIe would be millions of uncached
    reads; such a call is staged like any batch.  Bytes and verdicts for both sides of the 16 KiB gate, and the big
    call must not be absurdly slower than the small one."""
    import time
    sk = synth.random_bytes((1, 32), 0x7c01)
    pub, priv = api.ed25519_CreateKeyPair(sk)
    took = {}
    for mlen in (100, 16000, 17000, 1 << 20):
        msg = synth.random_bytes((1, mlen), 0x7c02 + mlen)
        api.ed25519_SignMessage(priv, msg)
        t0 = time.perf_counter()
        sig = api.ed25519_SignMessage(priv, msg)
        took[mlen] = time.perf_counter() - t0
        assert np.array_equal(sig, oracle.ed25519_sign(priv, msg)), mlen
        assert api.ed25519_VerifySignature(sig, pub, msg)[0] == 1
        msg[0, mlen // 2] ^= 1
        assert api.ed25519_VerifySignature(sig, pub, msg)[0] == 0
    assert took[1 << 20] < 2.0, took                                    # a lone lane hashes 1 MiB twice: tens of ms, not minutes


@pytest.mark.gpu
@pytest.mark.parametrize("done_word", ["1", "0"])
def test_single_calls_return_on_the_completion_word(done_word):
    """A call of ONE element through the reference's prototypes returns when the call's last kernel has stored the call's
    sequence number into pinned host memory behind its results (capi_common.hpp: ThreadState::done_word; 4.6 us earlier than the
    runtime's event, profiles/r06_launch_latency.txt) -- so a few hundred back-to-back calls with FRESH inputs each, every
    operation in turn, must each return their own results (a word seen early, or a stale sequence number, would hand back the
    previous call's bytes), from two threads at once; C25519_AMD_DONE_WORD=0 (the event path) gives the same bytes.  Verification
    includes keys off the curve and corrupted signatures: the slow-list kernel is that call's last kernel and signals either way."""
    code = r'''
import ctypes as C, os, sys, threading
import numpy as np
sys.path.insert(0, os.path.join(%r, "tests"))
sys.path.insert(0, %r)
from oracle_lib import Oracle
from curve25519_amd import _lib, synth
L = _lib.load()
orc = Oracle()
buf = lambda a: (C.c_ubyte * a.size).from_buffer_copy(a.tobytes())
def worker(seed, errors):
    try:
        n = 96
        sk, pk = synth.x25519_inputs(n, seed_shift=seed)
        exp, exp_sk = orc.x25519_shared(pk, sk)
        esk, msg = synth.ed25519_inputs(n, seed_shift=seed + 1)
        epub, epriv = orc.ed25519_keypair(esk)
        esig = orc.ed25519_sign(epriv, msg)
        bsig, bmsg, bad = synth.corrupt_for_verify(esig, msg)
        keys = epub.copy()
        keys[::5] = synth.random_bytes((n, 32), seed + 2)[::5]        # garbage keys: the slow list gets its element
        everd = orc.ed25519_verify(bsig, keys, bmsg)
        pub_fast_exp, _ = orc.x25519_public(sk, fast=True)
        for i in range(n):
            out, s = (C.c_ubyte * 32)(), buf(sk[i])
            L.curve25519_dh_CreateSharedKey(out, buf(pk[i]), s)
            assert bytes(out) == exp[i].tobytes() and bytes(s) == exp_sk[i].tobytes(), ("x25519", i)
            s = buf(sk[i])
            L.curve25519_dh_CalculatePublicKey_fast(out, s)
            assert bytes(out) == pub_fast_exp[i].tobytes(), ("public_fast", i)
            pub, priv, sig = (C.c_ubyte * 32)(), (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
            L.ed25519_CreateKeyPair(pub, priv, None, buf(esk[i]))
            assert bytes(pub) == epub[i].tobytes() and bytes(priv) == epriv[i].tobytes(), ("keypair", i)
            L.ed25519_SignMessage(sig, priv, None, buf(msg[i]), msg.shape[1])
            assert bytes(sig) == esig[i].tobytes(), ("sign", i)
            v = L.ed25519_VerifySignature(buf(bsig[i]), buf(keys[i]), buf(bmsg[i]), bmsg.shape[1])
            assert v == int(everd[i]), ("verify", i, v, int(everd[i]))
            ctx = L.ed25519_Verify_Init(None, buf(epub[i]))
            v = L.ed25519_Verify_Check(ctx, buf(bsig[i]), buf(bmsg[i]), bmsg.shape[1])
            L.ed25519_Verify_Finish(ctx)
            assert v == int(orc.ed25519_verify(bsig[i:i + 1], epub[i:i + 1], bmsg[i:i + 1])[0]), ("check", i)
        # a call of one carries its key and a message of up to 64 bytes in the kernel's arguments (lanes.cuh: CallWords): both sides of that
        for mlen in (0, 1, 31, 63, 64, 65, 100, 257):
            m1 = synth.random_bytes((1, max(mlen, 1)), seed + 3 + mlen)[:, :mlen]
            sig = (C.c_ubyte * 64)()
            L.ed25519_SignMessage(sig, buf(epriv[0]), None, buf(m1[0]) if mlen else None, mlen)
            assert bytes(sig) == orc.ed25519_sign(epriv[:1], m1)[0].tobytes(), ("sign, message length", mlen)
            assert L.ed25519_VerifySignature(sig, buf(epub[0]), buf(m1[0]) if mlen else None, mlen) == 1, ("verify, message length", mlen)
    except BaseException as e:
        errors.append(repr(e))
errors = []
ts = [threading.Thread(target=worker, args=(0x600 + 16 * t, errors)) for t in range(2)]
[t.start() for t in ts]; [t.join() for t in ts]
assert not errors, errors
print("ok")
''' % (ROOT, ROOT)
    env = dict(os.environ, C25519_AMD_DONE_WORD=done_word)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
