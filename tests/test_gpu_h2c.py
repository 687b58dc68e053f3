"""GPU suite (MI355X): c25519_ExpandMessageXmd_*, ed25519_MapToCurve_*, ed25519_HashToCurve_*, ed25519_EncodeToCurve_*,
ristretto255_HashToGroup_* and ed25519_HashToScalar_*.  Every output must be the bytes of the big-integer model (tests/h2c_model.py,
pinned to RFC 9380's and RFC 9497's vectors by tests/test_h2c_model.py) on the case set the CPU tests share, in both forms; the
published vectors must come out of the device through the C ABI; the calls must write every row and nothing behind the last one,
leave their inputs alone and work on another stream; and RFC 9497's blind / evaluate / unblind chain must close on the device with
the group and scalar calls it was added for."""
import ctypes as C

import numpy as np
import pytest

import h2c_model as model
import test_h2c_model as published
from curve25519_amd import _lib

pytestmark = pytest.mark.gpu

# the launch edges: one lane, around a wave, around a workgroup of 256, several workgroups with a ragged last one
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
FILL = 0xA5
CALLS = {"hash_to_curve": "ed25519_HashToCurve", "encode_to_curve": "ed25519_EncodeToCurve", "hash_to_group": "ristretto255_HashToGroup",
         "hash_to_scalar": "ed25519_HashToScalar"}


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


def call_dev(api, name, msgs, dst, width=32):
    """<name>_dev on a device copy of the messages into rows pre-filled with FILL, one guard row behind them: the rows, with the
    messages unchanged and the guard untouched"""
    import torch
    n = len(msgs)
    d_msg = to_dev(msgs)
    d_out = torch.full((n + 1, width), FILL, dtype=torch.uint8, device=dev())
    getattr(api, name + "_dev")(d_out[:n], d_msg, dst)
    torch.cuda.synchronize()
    assert np.array_equal(d_msg.cpu().numpy(), msgs), "inputs are never written"
    out = d_out.cpu().numpy()
    assert (out[n] == FILL).all(), "nothing is written behind the last row"
    return out[:n]


def call_batch(lib, name, msgs, dst, width=32, extra=()):
    n, size = msgs.shape
    out, before = np.full((n + 1, width), FILL, np.uint8), msgs.copy()
    rc = getattr(lib, name + "_batch")(C.c_void_p(out.ctypes.data), C.c_void_p(msgs.ctypes.data) if size else None, size, dst, len(dst),
                                       *extra, n)
    assert rc == 0, lib.c25519_amd_last_error()
    assert np.array_equal(msgs, before) and (out[n] == FILL).all()
    return out[:n]


def one(lib, name, msg: bytes, dst: bytes) -> str:
    return call_batch(lib, name, np.frombuffer(msg, np.uint8).reshape(1, len(msg)).copy(), dst)[0].tobytes().hex()


@pytest.mark.parametrize("call", sorted(CALLS))
def test_case_set(api, call):
    """the whole case set through _dev and _batch: the model's bytes in both forms"""
    lib = _lib.load()
    for dst, size, msgs in model.case_set():
        want = model.expected(call, dst, msgs)
        got = call_dev(api, CALLS[call], msgs, dst)
        assert np.array_equal(got, want), (call, len(dst), size, got[0].tobytes().hex(), want[0].tobytes().hex())
        assert np.array_equal(call_batch(lib, CALLS[call], msgs, dst), want), (call, len(dst), size, "batch")
        assert np.array_equal(getattr(api, CALLS[call])(msgs, dst), want)


def test_case_set_expand_message_xmd(api):
    lib = _lib.load()
    for dst, size, msgs, n_bytes in model.xmd_cases():
        want = model.expected("xmd", dst, msgs, n_bytes)
        assert np.array_equal(call_dev(api, "c25519_ExpandMessageXmd", msgs, dst, n_bytes), want), (len(dst), size, n_bytes)
        assert np.array_equal(call_batch(lib, "c25519_ExpandMessageXmd", msgs, dst, n_bytes, (n_bytes,)), want), (len(dst), size, n_bytes)
    dst, size, msgs = model.case_set()[0]
    assert np.array_equal(api.c25519_ExpandMessageXmd(msgs, dst, 65), model.expected("xmd", dst, msgs, 65))


def test_case_set_map_to_curve(api):
    import torch
    u, want = model.map_inputs(), model.expected_map()
    d_u, d_p = to_dev(u), torch.full((len(u) + 1, 32), FILL, dtype=torch.uint8, device=dev())
    api.ed25519_MapToCurve_dev(d_p[:len(u)], d_u)
    torch.cuda.synchronize()
    got = d_p.cpu().numpy()
    assert np.array_equal(got[:-1], want) and (got[-1] == FILL).all() and np.array_equal(d_u.cpu().numpy(), u)
    copy = u.copy()
    assert np.array_equal(api.ed25519_MapToCurve(copy), want) and np.array_equal(copy, u)
    assert got[0].tobytes().hex() == "01" + "00" * 31, "u = 0 gives the identity"


def test_the_published_vectors_through_the_c_abi(api):
    lib = _lib.load()
    for msg, want in ((b"", "6b9a7312411d92f921c6f68ca0b6380730a1a4d982c507211a90964c394179ba"),
                      (b"abc", "0da749f12fbe5483eb066a5f595055679b976e93abe9be6f0f6318bce7aca8dc")):
        rows = np.frombuffer(msg, np.uint8).reshape(1, len(msg)).copy()
        got = call_batch(lib, "c25519_ExpandMessageXmd", rows, published.XMD_DST, 32, (32,))
        assert got[0].tobytes().hex() == want, "RFC 9380 K.3"
    for msg, (x, y) in published.RO_POINTS.items():
        want = (int(y, 16) | (int(x, 16) & 1) << 255).to_bytes(32, "little").hex()
        assert one(lib, "ed25519_HashToCurve", msg, published.RO_DST) == want, msg
    assert one(lib, "ed25519_HashToCurve", b"", published.RO_DST) == "21dc15e10253796df23a7699c8a383ea624cce88c52431f6be220b1a56c8a609"
    for msg, (x, y) in published.NU_POINTS.items():
        want = (int(y, 16) | (int(x, 16) & 1) << 255).to_bytes(32, "little").hex()
        assert one(lib, "ed25519_EncodeToCurve", msg, published.NU_DST) == want, msg
    ctx = model.oprf_context_string()
    assert one(lib, "ristretto255_HashToGroup", published.OPRF_INPUT, b"HashToGroup-" + ctx) == published.OPRF_ELEMENT
    derive = published.OPRF_SEED + len(published.OPRF_INFO).to_bytes(2, "big") + published.OPRF_INFO + b"\x00"
    assert one(lib, "ed25519_HashToScalar", derive, b"DeriveKeyPair" + ctx) == published.OPRF_SKS


@pytest.mark.parametrize("n", SIZES)
def test_sizes(api, n):
    """every call at n elements, cases of the set tiled to length -- a different handful for every n, a straddling and a
    word-aligned message length among them: every row is the model's, the guard row stays"""
    cases = model.case_set()
    start = SIZES.index(n) * 5
    picked = [cases[(start + k) % len(cases)] for k in range(4)] + [c for c in cases if (len(c[0]), c[1]) in ((16, 64), (62, 9))]
    reps = -(-n // model.ROWS_PER_CASE)
    lib = _lib.load()
    for i, (dst, size, msgs) in enumerate(picked):
        tiled = np.ascontiguousarray(np.tile(msgs, (reps, 1))[:n])
        for call, name in CALLS.items():
            want = np.tile(model.expected(call, dst, msgs), (reps, 1))[:n]
            assert np.array_equal(call_dev(api, name, tiled, dst), want), (call, n, len(dst), size)
            if i == 0:
                assert np.array_equal(call_batch(lib, name, tiled, dst), want), (call, n, "batch")
        want = np.tile(model.expected("xmd", dst, msgs, 129), (reps, 1))[:n]
        assert np.array_equal(call_dev(api, "c25519_ExpandMessageXmd", tiled, dst, 129), want), (n, len(dst), size)
    u = model.map_inputs()
    tiled = np.ascontiguousarray(np.tile(u, (-(-n // len(u)), 1))[:n])
    assert np.array_equal(api.ed25519_MapToCurve(tiled), np.tile(model.expected_map(), (-(-n // len(u)), 1))[:n])


def test_messages_of_no_bytes(api):
    """msg_size == 0: the device form takes a tensor of no columns (a NULL msg), the host form a NULL pointer"""
    import torch
    dst = model.make_dst(16)
    for call, name in CALLS.items():
        want = np.frombuffer({"hash_to_curve": model.hash_to_curve, "encode_to_curve": model.encode_to_curve,
                              "hash_to_group": model.hash_to_group, "hash_to_scalar": model.hash_to_scalar}[call](b"", dst), np.uint8)
        d_out = torch.full((5, 32), FILL, dtype=torch.uint8, device=dev())
        getattr(api, name + "_dev")(d_out, torch.zeros((5, 0), dtype=torch.uint8, device=dev()), dst)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == want).all(), call
        assert (getattr(api, name)(np.zeros((5, 0), np.uint8), dst) == want).all(), call


def test_another_stream_and_refused_calls(api):
    import torch
    lib = _lib.load()
    dst, size, msgs = next(c for c in model.case_set() if (len(c[0]), c[1]) == (62, 65))
    n = 300
    tiled = np.ascontiguousarray(np.tile(msgs, (100, 1)))
    d_msg = to_dev(tiled)
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        outs = {call: torch.full((n, 32), FILL, dtype=torch.uint8, device=dev()) for call in CALLS}
        for call, name in CALLS.items():
            getattr(api, name + "_dev")(outs[call], d_msg, dst)
    side.synchronize()
    for call in CALLS:
        assert np.array_equal(outs[call].cpu().numpy(), np.tile(model.expected(call, dst, msgs), (100, 1))), call
    d_out = torch.full((n, 64), FILL, dtype=torch.uint8, device=dev())
    p, m = C.c_void_p(d_out.data_ptr()), C.c_void_p(d_msg.data_ptr())
    for name in CALLS.values():
        assert getattr(lib, name + "_dev")(p, m, size, dst, 0, n, None) != 0 and b"dst_len" in lib.c25519_amd_last_error()
        assert getattr(lib, name + "_dev")(p, m, size, dst, 256, n, None) != 0
        assert getattr(lib, name + "_dev")(p, None, size, dst, len(dst), n, None) != 0 and b"null pointer" in lib.c25519_amd_last_error()
        assert getattr(lib, name + "_dev")(p, C.c_void_p(d_msg.data_ptr() + 8), size, dst, len(dst), n, None) != 0, "misaligned"
    assert lib.c25519_ExpandMessageXmd_dev(p, m, size, dst, len(dst), 0, n, None) != 0 and b"len_in_bytes" in lib.c25519_amd_last_error()
    assert lib.c25519_ExpandMessageXmd_dev(p, m, size, dst, len(dst), 16321, n, None) != 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all(), "a refused call writes nothing"


def test_device_calls_can_be_captured_into_a_hip_graph(api):
    """a *_dev call is one kernel whose uniform part travels in its arguments: nothing is allocated or copied on the stream, so it
    can be captured and replayed -- and the replay hashes under the DST of the capture, whatever the host buffer holds by then"""
    import torch
    dst, size, msgs = next(c for c in model.case_set() if (len(c[0]), c[1]) == (62, 9))
    n = 300
    tiled = np.ascontiguousarray(np.tile(msgs, (100, 1)))
    d_msg = to_dev(tiled)
    outs = {call: torch.full((n, 32), FILL, dtype=torch.uint8, device=dev()) for call in CALLS}
    side = torch.cuda.Stream(dev())
    tag = bytearray(dst)

    def step():
        for call, name in CALLS.items():
            getattr(api, name + "_dev")(outs[call], d_msg, tag)

    with torch.cuda.stream(side):
        step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    tag[:] = bytes(len(tag))
    for _ in range(2):
        for t in outs.values():
            t.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for call in CALLS:
            assert np.array_equal(outs[call].cpu().numpy(), np.tile(model.expected(call, dst, msgs), (100, 1))), call


def test_the_oprf_chain_on_the_device(api):
    """RFC 9497 A.1.1 end to end: HashToScalar derives skS, HashToGroup hashes the input, ristretto255_ScalarMult blinds and
    evaluates -- the vector's BlindedElement and EvaluationElement -- and ed25519_ScalarInvert takes the blind off again"""
    import torch
    ctx = model.oprf_context_string()
    u8 = lambda n, w=32: torch.full((n, w), FILL, dtype=torch.uint8, device=dev())  # noqa: E731
    i32 = lambda n: torch.zeros((n, 1), dtype=torch.int32, device=dev())  # noqa: E731
    derive = published.OPRF_SEED + len(published.OPRF_INFO).to_bytes(2, "big") + published.OPRF_INFO + b"\x00"
    d_sks, d_el, d_blinded, d_eval, d_inv, d_back, d_n = (u8(1) for _ in range(7))
    ok = [i32(1) for _ in range(4)]
    api.ed25519_HashToScalar_dev(d_sks, to_dev(np.frombuffer(derive, np.uint8).reshape(1, -1)), b"DeriveKeyPair" + ctx)
    api.ristretto255_HashToGroup_dev(d_el, to_dev(np.frombuffer(published.OPRF_INPUT, np.uint8).reshape(1, -1)), b"HashToGroup-" + ctx)
    d_blind = to_dev(np.frombuffer(bytes.fromhex(published.OPRF_BLIND), np.uint8).reshape(1, 32))
    api.ristretto255_ScalarMult_dev(d_blinded, ok[0], d_blind, d_el)
    api.ristretto255_ScalarMult_dev(d_eval, ok[1], d_sks, d_blinded)
    api.ed25519_ScalarInvert_dev(d_inv, ok[2], d_blind)
    api.ristretto255_ScalarMult_dev(d_back, ok[3], d_inv, d_blinded)
    api.ristretto255_ScalarMult_dev(d_n, ok[3], d_inv, d_eval)
    torch.cuda.synchronize()
    hexes = [t.cpu().numpy().tobytes().hex() for t in (d_sks, d_el, d_blinded, d_eval, d_back)]
    assert hexes == [published.OPRF_SKS, published.OPRF_ELEMENT, published.OPRF_BLINDED, published.OPRF_EVALUATION, published.OPRF_ELEMENT]
    assert all(int(t.cpu().numpy()[0, 0]) == 1 for t in ok)
    assert model.oprf_finalize(published.OPRF_INPUT, d_n.cpu().numpy().tobytes()).hex() == published.OPRF_OUTPUT


def test_hashed_points_are_torsion_free(api):
    """ed25519_ClassifyKey_dev on the outputs: HashToCurve and EncodeToCurve land in the prime-order subgroup, MapToCurve's raw
    points mostly do not"""
    import torch
    dst, size, msgs = next(c for c in model.case_set() if (len(c[0]), c[1]) == (16, 65))
    tiled = np.ascontiguousarray(np.tile(msgs, (22, 1)))
    tiled[:, 0] = np.arange(len(tiled))                     # 66 different messages
    d_msg = to_dev(tiled)
    want = api.KEY_DECODES | api.KEY_CANONICAL | api.KEY_TORSION_FREE
    for name in ("ed25519_HashToCurve", "ed25519_EncodeToCurve"):
        d_p = torch.full((len(tiled), 32), FILL, dtype=torch.uint8, device=dev())
        d_flags = torch.zeros((len(tiled), 1), dtype=torch.int32, device=dev())
        getattr(api, name + "_dev")(d_p, d_msg, dst)
        api.ed25519_ClassifyKey_dev(d_flags, d_p)
        torch.cuda.synchronize()
        assert (d_flags.cpu().numpy().reshape(-1) == want).all(), name
        assert len({r.tobytes() for r in d_p.cpu().numpy()}) == len(tiled)
    flags = api.ed25519_ClassifyKey(api.ed25519_MapToCurve(model.map_inputs()))
    assert (flags & api.KEY_DECODES).all() and ((flags & api.KEY_TORSION_FREE) == 0).sum() >= len(flags) // 2
