"""GPU suite (MI355X): ed25519_ScalarReduce_*, _ScalarAdd_*, _ScalarSub_*, _ScalarMul_*, _ScalarNegate_*, _ScalarComplement_*,
_ScalarMulAdd_*, _ScalarInvert_* and _ScalarIsCanonical_*.  Every output must be the bytes of the big-integer model
(tests/scalar_model.py, pinned by tests/test_scalar_model.py) on the case set the CPU tests share, at every size, at every group size
of the inversion and in both forms; the calls must write every row, leave their inputs alone, work in place and on another stream,
and close the loop with the group calls they were added for."""
import ctypes as C

import numpy as np
import pytest

import scalar_model as model
from curve25519_amd import _lib
from scalar_model import KS, L

pytestmark = pytest.mark.gpu

# 257 crosses a workgroup, 65 539 the built-in switch of the inversion's group size (K = 1 up to 65 536 elements, K = 8 above)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, 65539)
FILL = 0xA5
ELEMENTWISE = {"Reduce": ("w",), "Add": ("x", "y"), "Sub": ("x", "y"), "Mul": ("x", "y"), "Negate": ("x",), "Complement": ("x",),
               "MulAdd": ("x", "y", "z")}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def cases():
    return model.case_set()


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def filled(shape, dtype):
    """a device tensor of `dtype` over shape[0] rows of shape[1] bytes, every byte FILL: an unwritten row shows"""
    import torch
    t = torch.full(shape, FILL, dtype=torch.uint8, device=dev())
    return t if dtype == torch.uint8 else t.view(dtype)


def rows_differ(got, want):
    return np.flatnonzero((got != want).any(axis=1))


def elementwise_dev(api, name, inputs):
    """ed25519_Scalar<name>_dev on device copies of the inputs; the copies must come back unchanged"""
    import torch
    d_in = [to_dev(a) for a in inputs]
    d_r = filled((len(inputs[0]), 32), torch.uint8)
    getattr(api, f"ed25519_Scalar{name}_dev")(d_r, *d_in)
    torch.cuda.synchronize()
    for d, a in zip(d_in, inputs):
        assert np.array_equal(d.cpu().numpy(), a), "inputs are never written"
    return d_r.cpu().numpy()


def invert_dev(api, s):
    import torch
    n = len(s)
    d_s, d_r, d_ok = to_dev(s), filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
    api.ed25519_ScalarInvert_dev(d_r, d_ok, d_s)
    torch.cuda.synchronize()
    assert np.array_equal(d_s.cpu().numpy(), s), "inputs are never written"
    return d_r.cpu().numpy(), d_ok.cpu().numpy().reshape(n)


def canonical_dev(api, s):
    import torch
    d_ok = filled((len(s), 4), torch.int32)
    api.ed25519_ScalarIsCanonical_dev(d_ok, to_dev(s))
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().reshape(len(s))


@pytest.mark.parametrize("name", sorted(ELEMENTWISE))
def test_case_set_elementwise(api, cases, name):
    """the whole case set through _dev and _batch: the model's bytes in both forms"""
    inputs = [cases[k] for k in ELEMENTWISE[name]]
    want = cases[name.lower()]
    got = elementwise_dev(api, name, inputs)
    bad = rows_differ(got, want)
    assert not len(bad), [(int(i), [a[i].tobytes().hex() for a in inputs], got[i].tobytes().hex(), want[i].tobytes().hex()) for i in bad][:4]
    copies = [a.copy() for a in inputs]
    host = getattr(api, f"ed25519_Scalar{name}")(*copies)
    assert np.array_equal(host, want) and all(np.array_equal(a, b) for a, b in zip(copies, inputs))


def test_case_set_is_canonical(api, cases):
    assert np.array_equal(canonical_dev(api, cases["x"]), cases["canonical"])
    assert np.array_equal(api.ed25519_ScalarIsCanonical(cases["x"].copy()), cases["canonical"])


@pytest.mark.parametrize("k", KS + (3,))
def test_case_set_invert(api, cases, k):
    """the whole case set at group size k through _dev and _batch; k = 3 is outside the set and means the built-in choice; the tunable
    reads -1 afterwards"""
    with _lib.tunable("SC_INVERT_K", k):
        assert _lib.load().c25519_amd_tunable_get(b"SC_INVERT_K") == k
        recip, ok = invert_dev(api, cases["x"])
        assert np.array_equal(ok, cases["ok"]), np.flatnonzero(ok != cases["ok"])[:8]
        bad = rows_differ(recip, cases["recip"])
        assert not len(bad), [(int(i), cases["x"][i].tobytes().hex(), recip[i].tobytes().hex(), cases["recip"][i].tobytes().hex()) for i in bad][:4]
        assert not recip[cases["ok"] == 0].any() and set(np.unique(ok)) == {0, 1}
        copy = cases["x"].copy()
        host, host_ok = api.ed25519_ScalarInvert(copy)
        assert np.array_equal(host, cases["recip"]) and np.array_equal(host_ok, cases["ok"]) and np.array_equal(copy, cases["x"])
    assert _lib.load().c25519_amd_tunable_get(b"SC_INVERT_K") == -1, "the tunable is restored"


@pytest.mark.parametrize("n", SIZES)
def test_sizes(api, cases, n):
    """every call at n elements, the case set cycled to length, the inversion at every group size and at the built-in one: every row of
    buffers pre-filled with 0xA5 is the model's, in both forms"""
    lib = _lib.load()
    if n == 0:
        import torch
        one = filled((1, 64), torch.uint8)
        flag = filled((1, 4), torch.int32)
        p, q = C.c_void_p(one.data_ptr()), C.c_void_p(flag.data_ptr())
        host, hflag = np.full((1, 64), FILL, np.uint8), np.full(1, 0x25A5A5A5, np.int32)
        hp, hq = C.c_void_p(host.ctypes.data), C.c_void_p(hflag.ctypes.data)
        for name, inputs in ELEMENTWISE.items():
            assert getattr(lib, f"ed25519_Scalar{name}_dev")(p, *[p] * len(inputs), 0, None) == 0
            assert getattr(lib, f"ed25519_Scalar{name}_batch")(hp, *[hp] * len(inputs), 0) == 0
        assert lib.ed25519_ScalarInvert_dev(p, q, p, 0, None) == 0 and lib.ed25519_ScalarInvert_batch(hp, hq, hp, 0) == 0
        assert lib.ed25519_ScalarIsCanonical_dev(q, p, 0, None) == 0 and lib.ed25519_ScalarIsCanonical_batch(hq, hp, 0) == 0
        torch.cuda.synchronize()
        assert (one.cpu().numpy() == FILL).all() and (flag.cpu().numpy().view(np.uint8) == FILL).all(), "a call of nothing writes nothing"
        assert (host == FILL).all() and (hflag == 0x25A5A5A5).all()
        return
    for name, keys in ELEMENTWISE.items():
        inputs = [model.cycled(cases[k], n) for k in keys]
        want = model.cycled(cases[name.lower()], n)
        assert np.array_equal(elementwise_dev(api, name, inputs), want), name
        assert np.array_equal(getattr(api, f"ed25519_Scalar{name}")(*inputs), want), name
    x = model.cycled(cases["x"], n)
    want, want_ok = model.cycled(cases["recip"], n), model.cycled(cases["ok"], n)
    for k in KS + (-1,):
        with _lib.tunable("SC_INVERT_K", k):
            recip, ok = invert_dev(api, x)
            assert np.array_equal(ok, want_ok) and not len(rows_differ(recip, want)), k
    host, host_ok = api.ed25519_ScalarInvert(x)
    assert np.array_equal(host, want) and np.array_equal(host_ok, want_ok)
    assert np.array_equal(canonical_dev(api, x), model.cycled(cases["canonical"], n))
    assert np.array_equal(api.ed25519_ScalarIsCanonical(x), model.cycled(cases["canonical"], n))


def test_in_place(api, cases):
    """an output buffer may be exactly an input buffer: every call on every one of its 32-byte inputs, the inversion at every group
    size, in both forms"""
    import torch
    n = 1025
    for name, keys in ELEMENTWISE.items():
        if name == "Reduce":
            continue                                     # its input rows are 64 bytes
        inputs = [model.cycled(cases[k], n) for k in keys]
        want = model.cycled(cases[name.lower()], n)
        for which in range(len(inputs)):
            d_in = [to_dev(a) for a in inputs]
            getattr(api, f"ed25519_Scalar{name}_dev")(d_in[which], *d_in)
            torch.cuda.synchronize()
            assert np.array_equal(d_in[which].cpu().numpy(), want), (name, which)
            assert all(np.array_equal(d.cpu().numpy(), a) for j, (d, a) in enumerate(zip(d_in, inputs)) if j != which)
            h_in = [a.copy() for a in inputs]
            lib = _lib.load()
            ptrs = [C.c_void_p(a.ctypes.data) for a in h_in]
            assert getattr(lib, f"ed25519_Scalar{name}_batch")(ptrs[which], *ptrs, n) == 0
            assert np.array_equal(h_in[which], want), (name, which, "batch")
    x = model.cycled(cases["x"], n)
    want, want_ok = model.cycled(cases["recip"], n), model.cycled(cases["ok"], n)
    for k in KS:
        with _lib.tunable("SC_INVERT_K", k):
            d_s, d_ok = to_dev(x), filled((n, 4), torch.int32)
            api.ed25519_ScalarInvert_dev(d_s, d_ok, d_s)
            torch.cuda.synchronize()
            assert np.array_equal(d_s.cpu().numpy(), want) and np.array_equal(d_ok.cpu().numpy().reshape(n), want_ok), k
    h, h_ok = x.copy(), np.full(n, 7, np.int32)
    assert _lib.load().ed25519_ScalarInvert_batch(C.c_void_p(h.ctypes.data), C.c_void_p(h_ok.ctypes.data), C.c_void_p(h.ctypes.data), n) == 0
    assert np.array_equal(h, want) and np.array_equal(h_ok, want_ok)


def test_arguments_and_streams(api, cases):
    """a null or misaligned pointer is an argument error and writes nothing; a call on another stream gives the same bytes"""
    import torch
    lib = _lib.load()
    n = 4
    d_x, d_w = to_dev(cases["x"][:n]), to_dev(cases["w"][:n])
    d_r, d_ok = filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
    h_r, h_ok = np.full((n, 32), FILL, np.uint8), np.full(n, 0x25A5A5A5, np.int32)
    x, w = cases["x"][:n].copy(), cases["w"][:n].copy()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    calls = {"ed25519_ScalarInvert": ([p(d_r), p(d_ok), p(d_x)], [hp(h_r), hp(h_ok), hp(x)]),
             "ed25519_ScalarIsCanonical": ([p(d_ok), p(d_x)], [hp(h_ok), hp(x)])}
    for name, keys in ELEMENTWISE.items():
        src, hsrc = (d_w, w) if name == "Reduce" else (d_x, x)
        calls[f"ed25519_Scalar{name}"] = ([p(d_r)] + [p(src)] * len(keys), [hp(h_r)] + [hp(hsrc)] * len(keys))
    refused = []
    for name, (dev_args, host_args) in calls.items():
        for k in range(len(dev_args)):
            refused.append(getattr(lib, name + "_dev")(*[None if i == k else a for i, a in enumerate(dev_args)], n, None))
            assert b"null pointer" in lib.c25519_amd_last_error(), name
            refused.append(getattr(lib, name + "_batch")(*[None if i == k else a for i, a in enumerate(host_args)], n))
            assert b"null pointer" in lib.c25519_amd_last_error(), name
    assert all(rc != 0 for rc in refused)
    off = C.c_void_p(d_x.data_ptr() + 8)
    assert lib.ed25519_ScalarInvert_dev(p(d_r), p(d_ok), off, n, None) != 0, "a misaligned device pointer is refused"
    assert lib.ed25519_ScalarMul_dev(p(d_r), off, p(d_x), n, None) != 0
    torch.cuda.synchronize()
    for t in (d_r, d_ok):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all(), "a refused call writes nothing"
    assert (h_r == FILL).all() and (h_ok == 0x25A5A5A5).all()
    side = torch.cuda.Stream(device=dev())
    m = len(cases["x"])
    s_x, s_y, s_z, s_w = (to_dev(cases[k]) for k in ("x", "y", "z", "w"))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s_inv, s_ok, s_mul = filled((m, 32), torch.uint8), filled((m, 4), torch.int32), filled((m, 32), torch.uint8)
        s_ma, s_red = filled((m, 32), torch.uint8), filled((len(cases["w"]), 32), torch.uint8)
        api.ed25519_ScalarInvert_dev(s_inv, s_ok, s_x)
        api.ed25519_ScalarMul_dev(s_mul, s_x, s_y)
        api.ed25519_ScalarMulAdd_dev(s_ma, s_x, s_y, s_z)
        api.ed25519_ScalarReduce_dev(s_red, s_w)
    side.synchronize()
    assert np.array_equal(s_inv.cpu().numpy(), cases["recip"]) and np.array_equal(s_ok.cpu().numpy().reshape(m), cases["ok"])
    assert np.array_equal(s_mul.cpu().numpy(), cases["mul"]) and np.array_equal(s_ma.cpu().numpy(), cases["muladd"])
    assert np.array_equal(s_red.cpu().numpy(), cases["reduce"])


def test_round_trip_through_the_group(api):
    """the two halves together: for 64 seeded (r, P), ristretto255_ScalarMult(1/r, ristretto255_ScalarMult(r, P)) is P's bytes again,
    and ristretto255_ScalarMultBase(a b + c) == [a]([b]B) + [c]B through the existing calls"""
    rng = np.random.default_rng(0x5CA1AA)
    n = 64
    r = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    r[:, 31] &= 0x7F                                     # the group calls read the low 255 bits; the scalar calls all 256
    assert all(v % L for v in model.from_rows(r))
    p = api.ristretto255_FromHash(rng.integers(0, 256, (n, 64), dtype=np.uint8))
    r_inv, ok = api.ed25519_ScalarInvert(r)
    assert ok.all()
    blinded, ok1 = api.ristretto255_ScalarMult(r, p)
    back, ok2 = api.ristretto255_ScalarMult(r_inv, blinded)
    assert ok1.all() and ok2.all() and np.array_equal(back, p) and len(rows_differ(blinded, p)) == n
    a, b, c = (rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(3))
    for t in (a, b, c):
        t[:, 31] &= 0x7F
    abc = api.ed25519_ScalarMulAdd(a, b, c)
    assert np.array_equal(abc, model.to_rows([model.muladd(*v) for v in zip(*(model.from_rows(t) for t in (a, b, c)))]))
    bB = api.ristretto255_ScalarMultBase(b)
    abB, ok3 = api.ristretto255_ScalarMult(a, bB)
    total, ok4 = api.ristretto255_PointAdd(abB, api.ristretto255_ScalarMultBase(c))
    assert ok3.all() and ok4.all() and np.array_equal(api.ristretto255_ScalarMultBase(abc), total)
