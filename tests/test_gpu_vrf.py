"""GPU suite (MI355X): ed25519_VRF_Prove_*, ed25519_VRF_Verify_* and ed25519_VRF_ProofToHash_* (ECVRF-EDWARDS25519-SHA512-ELL2,
RFC 9381).  Every output must be the bytes of the big-integer model (tests/vrf_model.py, pinned to the RFC's examples by
tests/test_vrf_model.py) on the case set the CPU tests share, through the _dev forms, the _batch forms and the api wrappers; the RFC's
examples must come out of the device through the C ABI; keys from ed25519_CreateKeyPair must prove and verify; the calls must write
every row and nothing behind the last one, leave their inputs alone, work on another stream and replay from a captured graph; and
the proof must be the one the existing calls compose."""
import ctypes as C

import numpy as np
import pytest

import vrf_model as model
from curve25519_amd import _lib
from scalar_model import cycled

pytestmark = pytest.mark.gpu

# the launch edges: one lane, around a wave, around a workgroup of 256, several workgroups with a ragged last one
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
FILL = 0xA5


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).to(dev())


def filled(n, width):
    import torch
    return torch.full((n + 1, width), FILL, dtype=torch.uint8, device=dev())


def ok_rows(n):
    import torch
    return torch.full((n + 1, 1), 0x5A5A5A5A, dtype=torch.int32, device=dev())


def prove_dev(api, priv, alpha):
    """ed25519_VRF_Prove_dev into rows pre-filled with FILL, one guard row behind them: the proofs, with the inputs unchanged and
    the guard untouched"""
    import torch
    n = len(priv)
    d_priv, d_alpha, d_out = to_dev(priv), to_dev(alpha), filled(n, 80)
    api.ed25519_VRF_Prove_dev(d_out[:n], d_priv, d_alpha)
    torch.cuda.synchronize()
    assert np.array_equal(d_priv.cpu().numpy(), priv) and np.array_equal(d_alpha.cpu().numpy(), alpha), "inputs are never written"
    out = d_out.cpu().numpy()
    assert (out[n] == FILL).all(), "nothing is written behind the last row"
    return out[:n]


def verify_dev(api, pk, pi, alpha):
    import torch
    n = len(pk)
    d_in = [to_dev(pk), to_dev(pi), to_dev(alpha)]
    d_beta, d_ok = filled(n, 64), ok_rows(n)
    api.ed25519_VRF_Verify_dev(d_beta[:n], d_ok[:n], *d_in)
    torch.cuda.synchronize()
    for t, a in zip(d_in, (pk, pi, alpha)):
        assert np.array_equal(t.cpu().numpy(), a), "inputs are never written"
    beta, ok = d_beta.cpu().numpy(), d_ok.cpu().numpy().reshape(-1)
    assert (beta[n] == FILL).all() and ok[n] == 0x5A5A5A5A, "nothing is written behind the last row"
    return beta[:n], ok[:n]


def proof_to_hash_dev(api, pi):
    import torch
    n = len(pi)
    d_pi, d_beta, d_ok = to_dev(pi), filled(n, 64), ok_rows(n)
    api.ed25519_VRF_ProofToHash_dev(d_beta[:n], d_ok[:n], d_pi)
    torch.cuda.synchronize()
    assert np.array_equal(d_pi.cpu().numpy(), pi)
    beta, ok = d_beta.cpu().numpy(), d_ok.cpu().numpy().reshape(-1)
    assert (beta[n] == FILL).all() and ok[n] == 0x5A5A5A5A
    return beta[:n], ok[:n]


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


def prove_batch(lib, priv, alpha):
    n = len(priv)
    out, before = np.full((n + 1, 80), FILL, np.uint8), (priv.copy(), alpha.copy())
    rc = lib.ed25519_VRF_Prove_batch(ptr(out), ptr(priv), ptr(alpha), alpha.shape[1], n)
    assert rc == 0, lib.c25519_amd_last_error()
    assert np.array_equal(priv, before[0]) and np.array_equal(alpha, before[1]) and (out[n] == FILL).all()
    return out[:n]


def verify_batch(lib, pk, pi, alpha):
    n = len(pk)
    beta, ok = np.full((n + 1, 64), FILL, np.uint8), np.full(n + 1, 0x5A5A5A5A, np.int32)
    before = (pk.copy(), pi.copy(), alpha.copy())
    rc = lib.ed25519_VRF_Verify_batch(ptr(beta), ptr(ok), ptr(pk), ptr(pi), ptr(alpha), alpha.shape[1], n)
    assert rc == 0, lib.c25519_amd_last_error()
    assert all(np.array_equal(a, b) for a, b in zip((pk, pi, alpha), before)) and (beta[n] == FILL).all() and ok[n] == 0x5A5A5A5A
    return beta[:n], ok[:n]


def proof_to_hash_batch(lib, pi):
    n = len(pi)
    beta, ok = np.full((n + 1, 64), FILL, np.uint8), np.full(n + 1, 0x5A5A5A5A, np.int32)
    rc = lib.ed25519_VRF_ProofToHash_batch(ptr(beta), ptr(ok), ptr(pi), n)
    assert rc == 0, lib.c25519_amd_last_error()
    assert (beta[n] == FILL).all() and ok[n] == 0x5A5A5A5A
    return beta[:n], ok[:n]


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("alpha_len", model.ALPHA_LENGTHS)
def test_honest_rows(api, alpha_len):
    """the honest rows of one alpha length through _dev, _batch and the wrappers: the model's bytes in every form"""
    lib = _lib.load()
    h = model.honest(alpha_len)
    priv, pk, alpha, pi, beta = (np.array(h[k]) for k in ("priv", "pk", "alpha", "pi", "beta"))
    ones = np.ones(len(pi), np.int32)
    assert np.array_equal(prove_dev(api, priv, alpha), pi), alpha_len
    assert np.array_equal(prove_batch(lib, priv, alpha), pi), alpha_len
    assert np.array_equal(api.ed25519_VRF_Prove(priv, alpha), pi), alpha_len
    for got in (verify_dev(api, pk, pi, alpha), verify_batch(lib, pk, pi, alpha), api.ed25519_VRF_Verify(pk, pi, alpha),
                proof_to_hash_dev(api, pi), proof_to_hash_batch(lib, pi), api.ed25519_VRF_ProofToHash(pi)):
        assert same(got, (beta, ones)), alpha_len


def test_rejection_rows(api):
    """every rejection row in every form: ok and beta are the model's, rejected rows are all zero, every row is written"""
    lib = _lib.load()
    r = model.rejections()
    pk, pi, alpha = (np.array(r[k]) for k in ("pk", "pi", "alpha"))
    for got in (verify_dev(api, pk, pi, alpha), verify_batch(lib, pk, pi, alpha), api.ed25519_VRF_Verify(pk, pi, alpha)):
        bad = [lab for lab, g, w in zip(r["labels"], got[1], r["ok"]) if g != w]
        assert not bad, bad
        assert np.array_equal(got[0], r["beta"])
        assert not got[0][got[1] == 0].any(), "rejected rows are zeros"
    for got in (proof_to_hash_dev(api, pi), proof_to_hash_batch(lib, pi), api.ed25519_VRF_ProofToHash(pi)):
        bad = [lab for lab, g, w in zip(r["labels"], got[1], r["ok_hash"]) if g != w]
        assert not bad, bad
        assert np.array_equal(got[0], r["beta_hash"])
        assert not got[0][got[1] == 0].any()


def test_the_public_half_is_read_as_given(api):
    priv, alpha, pi = model.mixed_order_privs()
    assert np.array_equal(prove_dev(api, priv, alpha), pi)


def test_the_published_examples_through_the_c_abi(api):
    lib = _lib.load()
    for priv, pk, alpha, pi, beta in model.example_rows():
        a = np.frombuffer(alpha, np.uint8).reshape(1, len(alpha)).copy()
        got = prove_batch(lib, np.frombuffer(priv, np.uint8).reshape(1, 64).copy(), a)
        assert got.tobytes().hex() == pi.hex()
        b, ok = verify_batch(lib, np.frombuffer(pk, np.uint8).reshape(1, 32).copy(), got, a)
        assert ok.tolist() == [1] and b.tobytes().hex() == beta.hex()
        b, ok = proof_to_hash_batch(lib, got)
        assert ok.tolist() == [1] and b.tobytes().hex() == beta.hex()


def test_keys_from_create_key_pair(api):
    """key pairs from ed25519_CreateKeyPair: Prove takes its priv, Verify its pub; Verify and ProofToHash agree on beta, no two
    outputs are the same, and another key's proof is refused"""
    from curve25519_amd import synth
    n = 96
    pub, priv = api.ed25519_CreateKeyPair(synth.random_bytes((n, 32), 0x9381))
    alpha = synth.random_bytes((n, 21), 0x9382)
    pi = api.ed25519_VRF_Prove(priv, alpha)
    beta, ok = api.ed25519_VRF_Verify(pub, pi, alpha)
    beta2, ok2 = api.ed25519_VRF_ProofToHash(pi)
    assert ok.tolist() == [1] * n and ok2.tolist() == [1] * n and np.array_equal(beta, beta2)
    assert len({b.tobytes() for b in beta}) == n
    assert model.verify(pub[0].tobytes(), pi[0].tobytes(), alpha[0].tobytes()) == (beta[0].tobytes(), 1)
    beta, ok = api.ed25519_VRF_Verify(np.roll(pub, 1, axis=0), pi, alpha)
    assert not ok.any() and not beta.any()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(api, n):
    """every call at n elements, the rows of the set cycled to length: every row is the model's, the guard row stays"""
    lib = _lib.load()
    h, r = model.honest(model.REJECT_ALPHA), model.rejections()
    priv, alpha, pi = cycled(h["priv"], n), cycled(h["alpha"], n), cycled(h["pi"], n)
    assert np.array_equal(prove_dev(api, priv, alpha), pi)
    pk, rpi, ralpha = cycled(r["pk"], n), cycled(r["pi"], n), cycled(r["alpha"], n)
    want = (cycled(r["beta"], n), cycled(r["ok"], n))
    assert same(verify_dev(api, pk, rpi, ralpha), want)
    want_hash = (cycled(r["beta_hash"], n), cycled(r["ok_hash"], n))
    assert same(proof_to_hash_dev(api, rpi), want_hash)
    if n in (65, 1000):
        assert np.array_equal(prove_batch(lib, priv, alpha), pi)
        assert same(verify_batch(lib, pk, rpi, ralpha), want)
        assert same(proof_to_hash_batch(lib, rpi), want_hash)


def test_alpha_of_no_bytes(api):
    """alpha_size == 0: the device form takes a tensor of no columns (a NULL alpha), the host form a NULL pointer"""
    h = model.honest(0)
    priv, pk, alpha, pi, beta = (cycled(h[k], 5) for k in ("priv", "pk", "alpha", "pi", "beta"))
    assert alpha.shape == (5, 0)
    assert np.array_equal(prove_dev(api, priv, alpha), pi)
    assert same(verify_dev(api, pk, pi, alpha), (beta, np.ones(5, np.int32)))
    assert np.array_equal(api.ed25519_VRF_Prove(priv, alpha), pi)


def test_another_stream_and_refused_calls(api):
    import torch
    lib = _lib.load()
    n = 300
    h = model.honest(53)
    priv, pk, alpha, pi, beta = (cycled(h[k], n) for k in ("priv", "pk", "alpha", "pi", "beta"))
    d_priv, d_pk, d_alpha, d_pi = to_dev(priv), to_dev(pk), to_dev(alpha), to_dev(pi)
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_out, d_beta, d_beta2, d_ok, d_ok2 = filled(n, 80), filled(n, 64), filled(n, 64), ok_rows(n), ok_rows(n)
        api.ed25519_VRF_Prove_dev(d_out[:n], d_priv, d_alpha)
        api.ed25519_VRF_Verify_dev(d_beta[:n], d_ok[:n], d_pk, d_out[:n], d_alpha)
        api.ed25519_VRF_ProofToHash_dev(d_beta2[:n], d_ok2[:n], d_out[:n])
    side.synchronize()
    assert np.array_equal(d_out.cpu().numpy()[:n], pi)
    assert np.array_equal(d_beta.cpu().numpy()[:n], beta) and np.array_equal(d_beta2.cpu().numpy()[:n], beta)
    assert (d_ok.cpu().numpy()[:n] == 1).all() and (d_ok2.cpu().numpy()[:n] == 1).all()
    d_out = filled(n, 80)
    o, k = C.c_void_p(d_out.data_ptr()), C.c_void_p(d_ok.data_ptr())
    p, a, q = C.c_void_p(d_priv.data_ptr()), C.c_void_p(d_alpha.data_ptr()), C.c_void_p(d_pi.data_ptr())
    assert lib.ed25519_VRF_Prove_dev(o, p, None, 53, n, None) != 0 and b"null pointer" in lib.c25519_amd_last_error()
    assert lib.ed25519_VRF_Prove_dev(o, C.c_void_p(d_priv.data_ptr() + 8), a, 53, n, None) != 0, "misaligned"
    assert lib.ed25519_VRF_Verify_dev(o, k, p, None, a, 53, n, None) != 0 and b"null pointer" in lib.c25519_amd_last_error()
    assert lib.ed25519_VRF_ProofToHash_dev(o, k, C.c_void_p(d_pi.data_ptr() + 4), n, None) != 0, "misaligned"
    assert lib.ed25519_VRF_ProofToHash_dev(C.c_void_p(pi.ctypes.data), k, q, n, None) != 0, "a host pointer"
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all(), "a refused call writes nothing"


def test_device_calls_can_be_captured_into_a_hip_graph(api):
    """a *_dev call of each kind is one kernel whose uniform part travels in its arguments: nothing is allocated or copied on the
    stream, so it can be captured, and the replay writes the same bytes"""
    import torch
    n = 300
    h = model.honest(36)
    priv, pk, alpha, pi, beta = (cycled(h[k], n) for k in ("priv", "pk", "alpha", "pi", "beta"))
    d_priv, d_pk, d_alpha = to_dev(priv), to_dev(pk), to_dev(alpha)
    d_out, d_beta, d_beta2, d_ok, d_ok2 = filled(n, 80), filled(n, 64), filled(n, 64), ok_rows(n), ok_rows(n)
    side = torch.cuda.Stream(dev())

    def step():
        api.ed25519_VRF_Prove_dev(d_out[:n], d_priv, d_alpha)
        api.ed25519_VRF_Verify_dev(d_beta[:n], d_ok[:n], d_pk, d_out[:n], d_alpha)
        api.ed25519_VRF_ProofToHash_dev(d_beta2[:n], d_ok2[:n], d_out[:n])

    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    for _ in range(2):
        for t in (d_out, d_beta, d_beta2):
            t.fill_(FILL)
        d_ok.fill_(7)
        d_ok2.fill_(7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[:n], pi) and (d_out.cpu().numpy()[n] == FILL).all()
        assert np.array_equal(d_beta.cpu().numpy()[:n], beta) and np.array_equal(d_beta2.cpu().numpy()[:n], beta)
        assert (d_ok.cpu().numpy()[:n] == 1).all() and (d_ok2.cpu().numpy()[:n] == 1).all()


def test_the_composed_path_gives_the_same_proof(api):
    """the proof from the calls a caller had before -- ed25519_EncodeToCurve_dev on pk || alpha, ed25519_ScalarMult_noclamp_dev twice,
    ed25519_ScalarMultBase_noclamp_dev, ed25519_ScalarMulAdd_dev, with x, k and c from the model where the host hashes stood -- is
    ed25519_VRF_Prove_dev's"""
    import torch
    rows = [(model.honest(a)["priv"][j].tobytes(), model.honest(a)["alpha"][j].tobytes()) for a in (9, 52) for j in range(2)]
    for alpha_len in (9, 52):
        sel = [(p, a) for p, a in rows if len(a) == alpha_len]
        n = len(sel)
        priv = np.stack([np.frombuffer(p, np.uint8) for p, _ in sel])
        alpha = np.stack([np.frombuffer(a, np.uint8) for _, a in sel])
        parts = [model.prove_parts(p, a) for p, a in sel]
        le = lambda v: np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)  # noqa: E731
        d_x, d_k, d_c = (to_dev(np.stack([le(q[name]) for q in parts])) for name in ("x", "k", "c"))
        u8 = lambda: torch.full((n, 32), FILL, dtype=torch.uint8, device=dev())  # noqa: E731
        d_h, d_gamma, d_u, d_v, d_s = (u8() for _ in range(5))
        d_ok = torch.zeros((n, 1), dtype=torch.int32, device=dev())
        api.ed25519_EncodeToCurve_dev(d_h, to_dev(np.concatenate([priv[:, 32:], alpha], axis=1)), model.DST)
        api.ed25519_ScalarMult_dev(d_gamma, d_ok, d_x, d_h, clamp=False)
        api.ed25519_ScalarMultBase_dev(d_u, d_k, clamp=False)
        api.ed25519_ScalarMult_dev(d_v, d_ok, d_k, d_h, clamp=False)
        api.ed25519_ScalarMulAdd_dev(d_s, d_c, d_x, d_k)
        torch.cuda.synchronize()
        composed = np.concatenate([d_gamma.cpu().numpy(), d_c.cpu().numpy()[:, :16], d_s.cpu().numpy()], axis=1)
        for q, h_row, u_row, v_row in zip(parts, d_h.cpu().numpy(), d_u.cpu().numpy(), d_v.cpu().numpy()):
            assert (h_row.tobytes(), u_row.tobytes(), v_row.tobytes()) == (q["H"], q["U"], q["V"])
        assert np.array_equal(composed, prove_dev(api, priv, alpha)), alpha_len
