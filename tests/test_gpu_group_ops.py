"""GPU suite (MI355X): ed25519_ScalarMult[_noclamp]_*, ed25519_ScalarMultBase[_noclamp]_*, ed25519_PointAdd_* and ed25519_PointSub_*.
Every output must be the bytes of the big-integer model of the stated rule (tests/group_model.py) on the case set the CPU tests
share, at every window width of the variable-base walk, at every size and in both forms; the calls must agree with the reference's
own bytes (the golden key pairs, the oracle's X25519) and with each other, and must leave the caller's scalar bytes alone."""
import ctypes as C
import os

import numpy as np
import pytest

import group_model as model
import key_model
from curve25519_amd import _lib
from oracle_lib import Oracle
from vectors import L

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 4097)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_1024.npz")
FILL = 0xA5
NEUTRAL_ENC = (1).to_bytes(32, "little")
EDGE_LABELS = ("mixed order", "small order", "y >= p", "x = 0 with the sign bit", "off the curve", "predicate boundary")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def cases():
    """the shared case set with the model's answers, clamped and not: about 200 pairs, the pool of the size tests too"""
    sc, pt, labels = model.case_set()
    want = {clamp: model.expected_scalarmult(sc, pt, clamp) for clamp in (True, False)}
    base = {clamp: model.expected_base(sc, clamp) for clamp in (True, False)}
    edge = np.flatnonzero(np.isin(np.array(labels), EDGE_LABELS))
    assert 150 <= len(sc) <= 260 and len(edge) > 100
    return sc, pt, labels, want, base, edge


@pytest.fixture(scope="module")
def add_cases():
    p, q, names = model.add_cases()
    return p, q, names, {sub: model.expected_add(p, q, sub) for sub in (False, True)}


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


def scalarmult_dev(api, sc, pt, clamp):
    import torch
    n = len(sc)
    d_sc, d_q, d_ok = to_dev(sc), filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
    api.ed25519_ScalarMult_dev(d_q, d_ok, d_sc, to_dev(pt), clamp=clamp)
    torch.cuda.synchronize()
    assert np.array_equal(d_sc.cpu().numpy(), sc), "the scalar bytes are not written"
    return d_q.cpu().numpy(), d_ok.cpu().numpy().reshape(n)


def base_dev(api, sc, clamp):
    import torch
    d_sc, d_q = to_dev(sc), filled((len(sc), 32), torch.uint8)
    api.ed25519_ScalarMultBase_dev(d_q, d_sc, clamp=clamp)
    torch.cuda.synchronize()
    assert np.array_equal(d_sc.cpu().numpy(), sc), "the scalar bytes are not written"
    return d_q.cpu().numpy()


def add_dev(api, p, q, sub):
    import torch
    n = len(p)
    d_r, d_ok = filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
    (api.ed25519_PointSub_dev if sub else api.ed25519_PointAdd_dev)(d_r, d_ok, to_dev(p), to_dev(q))
    torch.cuda.synchronize()
    return d_r.cpu().numpy(), d_ok.cpu().numpy().reshape(n)


def rows_differ(got, want):
    return np.flatnonzero((got != want).any(axis=1))


def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


@pytest.mark.parametrize("w", model.WINDOWS)
def test_case_set(api, cases, w):
    """the whole case set through _dev and _batch at window width w, clamped and not: the model's bytes in both forms"""
    sc, pt, labels, want, base, _ = cases
    with _lib.tunable("SCALARMULT_WINDOW", w):
        for clamp in (True, False):
            q, ok = want[clamp]
            got, got_ok = scalarmult_dev(api, sc, pt, clamp)
            assert np.array_equal(got_ok, ok), [(i, labels[i]) for i in np.flatnonzero(got_ok != ok)][:8]
            bad = rows_differ(got, q)
            assert not len(bad), [(int(i), labels[i], sc[i].tobytes().hex(), got[i].tobytes().hex(), q[i].tobytes().hex()) for i in bad][:4]
            before = sc.copy()
            host, host_ok = api.ed25519_ScalarMult(sc, pt, clamp=clamp)
            assert np.array_equal(host, q) and np.array_equal(host_ok, ok) and np.array_equal(sc, before)
            assert not got[ok == 0].any() and set(np.unique(got_ok)) == {0, 1}
    assert _lib.load().c25519_amd_tunable_get(b"SCALARMULT_WINDOW") == -1, "the tunable is restored"


def test_case_set_base_add_sub(api, cases, add_cases):
    sc, _, _, _, base, _ = cases
    for clamp in (True, False):
        assert not len(rows_differ(base_dev(api, sc, clamp), base[clamp]))
        before = sc.copy()
        assert np.array_equal(api.ed25519_ScalarMultBase(sc, clamp=clamp), base[clamp]) and np.array_equal(sc, before)
    p, q, names, want = add_cases
    for sub in (False, True):
        r, ok = want[sub]
        got, got_ok = add_dev(api, p, q, sub)
        assert np.array_equal(got_ok, ok), [(i, names[i]) for i in np.flatnonzero(got_ok != ok)][:8]
        bad = rows_differ(got, r)
        assert not len(bad), [(int(i), names[i], got[i].tobytes().hex(), r[i].tobytes().hex()) for i in bad][:4]
        host, host_ok = (api.ed25519_PointSub if sub else api.ed25519_PointAdd)(p, q)
        assert np.array_equal(host, r) and np.array_equal(host_ok, ok)
        assert not got[ok == 0].any()


def tiled(cases, n):
    """n rows of the pool in a seeded permutation, edge pairs in the first and last rows and on both sides of every 64-lane boundary"""
    sc, _, _, _, _, edge = cases
    rng = np.random.default_rng(0x6A + n)
    idx = np.concatenate([rng.permutation(len(sc)) for _ in range(n // len(sc) + 1)])[:n]
    at = sorted({0, n - 1} | {p for b in range(64, n, 64) for p in (b - 1, b)})
    idx[at] = edge[(np.arange(len(at)) * 7 + n) % len(edge)]
    return idx


def check_size(api, cases, add_cases, n, widths):
    sc, pt, labels, want, base, _ = cases
    idx = tiled(cases, n)
    s, p = sc[idx], pt[idx]
    for w in widths:
        with _lib.tunable("SCALARMULT_WINDOW", w):
            for clamp in (True, False):
                q, ok = want[clamp]
                got, got_ok = scalarmult_dev(api, s, p, clamp)
                assert np.array_equal(got_ok, ok[idx]) and not len(rows_differ(got, q[idx])), (w, clamp)
    for clamp in (True, False):
        q, ok = want[clamp]
        host, host_ok = api.ed25519_ScalarMult(s, p, clamp=clamp)
        assert np.array_equal(host_ok, ok[idx]) and np.array_equal(host, q[idx])
        assert np.array_equal(base_dev(api, s, clamp), base[clamp][idx])
        assert np.array_equal(api.ed25519_ScalarMultBase(s, clamp=clamp), base[clamp][idx])
    ap, aq, _, awant = add_cases
    rng = np.random.default_rng(0xADD + n)
    j = rng.integers(0, len(ap), n)
    for sub in (False, True):
        r, ok = awant[sub]
        got, got_ok = add_dev(api, ap[j], aq[j], sub)
        assert np.array_equal(got_ok, ok[j]) and np.array_equal(got, r[j])
        host, host_ok = (api.ed25519_PointSub if sub else api.ed25519_PointAdd)(ap[j], aq[j])
        assert np.array_equal(host_ok, ok[j]) and np.array_equal(host, r[j])


@pytest.mark.parametrize("n", SIZES)
def test_sizes(api, cases, add_cases, n):
    """every call at n elements, the variable-base walk at every width: every row of buffers pre-filled with 0xA5 is the model's"""
    check_size(api, cases, add_cases, n, model.WINDOWS)


def test_size_65537_at_the_built_in_width(api, cases, add_cases):
    check_size(api, cases, add_cases, 65537, (-1,))


def test_x25519_relation(api, cases):
    """for clamped scalars and every decodable case point: u of ScalarMult's point is curve25519_dh_CreateSharedKey of u(P), by this
    library's ladder and by the oracle's"""
    keys, labels = key_model.case_set()
    pts = np.stack([k for k in keys if key_model.decode(k.tobytes())[0] is not None])
    rng = np.random.default_rng(0x0DD5)
    sc = np.stack([np.frombuffer(key_model.clamp(rng.integers(0, 256, 32, dtype=np.uint8).tobytes()), np.uint8) for _ in pts])
    q, ok = api.ed25519_ScalarMult(sc, pts)
    assert ok.all()
    u_in = np.stack([np.frombuffer(model.montgomery_u_of(p.tobytes()), np.uint8) for p in pts])
    u_out = np.stack([np.frombuffer(model.montgomery_u_of(r.tobytes()), np.uint8) for r in q])
    ours, _ = api.curve25519_dh_CreateSharedKey(u_in, sc)
    theirs, _ = Oracle().x25519_shared(u_in, sc)
    assert np.array_equal(ours, theirs)
    assert np.array_equal(u_out, theirs), [int(i) for i in rows_differ(u_out, theirs)][:8]
    assert theirs.any(axis=1).sum() > 40
    q2, ok2 = api.ed25519_ScalarMult(sc, pts, clamp=False)
    assert np.array_equal(q2, q) and ok2.all(), "a clamped scalar is its own low 255 bits"


def test_base_relations(api):
    """ScalarMult on enc(B) is ScalarMultBase; [s]B = [s + L]B; the golden public keys; (a + b) mod L; P - P; honest outputs"""
    rng = np.random.default_rng(0xBA5E)
    n = 96
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x3F                                        # s < 2^254, so s + L < 2^255
    base_pt = np.tile(np.frombuffer(model.BASE, np.uint8), (n, 1))
    want = api.ed25519_ScalarMultBase(sc, clamp=False)
    for w in model.WINDOWS:
        with _lib.tunable("SCALARMULT_WINDOW", w):
            q, ok = api.ed25519_ScalarMult(sc, base_pt, clamp=False)
            assert ok.all() and np.array_equal(q, want), w
            q, ok = api.ed25519_ScalarMult(sc, base_pt)
            assert ok.all() and np.array_equal(q, api.ed25519_ScalarMultBase(sc)), w
    plus_l = np.stack([le32(int.from_bytes(s.tobytes(), "little") + L) for s in sc])
    assert np.array_equal(api.ed25519_ScalarMultBase(plus_l, clamp=False), want)
    for i in range(0, n, 12):
        assert want[i].tobytes() == model.scalarmult_base(sc[i].tobytes(), False), i
    a, b = sc[: n // 2], sc[n // 2:]
    total = np.stack([le32((int.from_bytes(x.tobytes(), "little") + int.from_bytes(y.tobytes(), "little")) % L) for x, y in zip(a, b)])
    r, ok = api.ed25519_PointAdd(want[: n // 2], want[n // 2:])
    assert ok.all() and np.array_equal(r, api.ed25519_ScalarMultBase(total, clamp=False))
    diff = np.stack([le32((int.from_bytes(x.tobytes(), "little") - int.from_bytes(y.tobytes(), "little")) % L) for x, y in zip(a, b)])
    r, ok = api.ed25519_PointSub(want[: n // 2], want[n // 2:])
    assert ok.all() and np.array_equal(r, api.ed25519_ScalarMultBase(diff, clamp=False))
    r, ok = api.ed25519_PointSub(want, want)
    assert ok.all() and all(x.tobytes() == NEUTRAL_ENC for x in r)
    assert np.array_equal(api.ed25519_ClassifyKey(want), np.full(n, 11, np.uint32))
    z = np.load(GOLDEN)
    seeds = z["ed_sk"]
    a = np.stack([np.frombuffer(model.seed_scalar(s.tobytes()), np.uint8) for s in seeds])
    assert np.array_equal(api.ed25519_ScalarMultBase(a), z["ed_pub"])
    assert np.array_equal(base_dev(api, a, False), z["ed_pub"])
    q, ok = api.ed25519_ScalarMult(a[:64], z["ed_pub"][64:128])
    assert ok.all() and np.array_equal(api.ed25519_ClassifyKey(q), np.full(64, 11, np.uint32))


def test_arguments(api, cases):
    """n == 0 returns 0 and writes nothing, a null or misaligned pointer is an argument error, a call on another stream gives the
    same bytes"""
    import torch
    sc, pt, labels, want, base, _ = cases
    L_ = _lib.load()
    d_sc, d_pt = to_dev(sc), to_dev(pt)
    d_q, d_ok = filled((4, 32), torch.uint8), filled((4, 4), torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    h_q, h_ok = np.full((4, 32), FILL, np.uint8), np.full(4, 0x25A5A5A5, np.int32)
    four = ("ed25519_ScalarMult", "ed25519_ScalarMult_noclamp", "ed25519_PointAdd", "ed25519_PointSub")
    two = ("ed25519_ScalarMultBase", "ed25519_ScalarMultBase_noclamp")
    for name in four:
        assert getattr(L_, name + "_dev")(p(d_q), p(d_ok), p(d_sc), p(d_pt), 0, None) == 0
        assert getattr(L_, name + "_batch")(hp(h_q), hp(h_ok), hp(sc), hp(pt), 0) == 0
    for name in two:
        assert getattr(L_, name + "_dev")(p(d_q), p(d_sc), 0, None) == 0
        assert getattr(L_, name + "_batch")(hp(h_q), hp(sc), 0) == 0
    refused = []
    for name in four:
        dev_args, host_args = [p(d_q), p(d_ok), p(d_sc), p(d_pt)], [hp(h_q), hp(h_ok), hp(sc), hp(pt)]
        for k in range(4):
            refused.append(getattr(L_, name + "_dev")(*[None if i == k else a for i, a in enumerate(dev_args)], 4, None))
            assert b"null pointer" in L_.c25519_amd_last_error()
            refused.append(getattr(L_, name + "_batch")(*[None if i == k else a for i, a in enumerate(host_args)], 4))
            assert b"null pointer" in L_.c25519_amd_last_error()
    for name in two:
        for k in range(2):
            refused.append(getattr(L_, name + "_dev")(*[None if i == k else a for i, a in enumerate([p(d_q), p(d_sc)])], 4, None))
            assert b"null pointer" in L_.c25519_amd_last_error()
            refused.append(getattr(L_, name + "_batch")(*[None if i == k else a for i, a in enumerate([hp(h_q), hp(sc)])], 4))
            assert b"null pointer" in L_.c25519_amd_last_error()
    assert all(rc != 0 for rc in refused)
    off = C.c_void_p(d_sc.data_ptr() + 8)
    assert L_.ed25519_ScalarMult_dev(p(d_q), p(d_ok), off, p(d_pt), 4, None) != 0, "a misaligned device pointer is refused"
    assert L_.ed25519_ScalarMultBase_dev(p(d_q), off, 4, None) != 0
    assert L_.ed25519_PointAdd_dev(p(d_q), p(d_ok), p(d_pt), off, 4, None) != 0
    torch.cuda.synchronize()
    for t in (d_q, d_ok):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all(), "a refused call and a call of nothing write nothing"
    assert (h_q == FILL).all() and (h_ok == 0x25A5A5A5).all()
    assert np.array_equal(d_sc.cpu().numpy(), sc)
    side = torch.cuda.Stream(device=dev())
    n = len(sc)
    with torch.cuda.stream(side):
        s_q, s_ok, s_b = filled((n, 32), torch.uint8), filled((n, 4), torch.int32), filled((n, 32), torch.uint8)
        s_r, s_rok = filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
        api.ed25519_ScalarMult_dev(s_q, s_ok, d_sc, d_pt, clamp=False)
        api.ed25519_ScalarMultBase_dev(s_b, d_sc)
        api.ed25519_PointAdd_dev(s_r, s_rok, d_pt, d_pt)
    side.synchronize()
    q, ok = want[False]
    assert np.array_equal(s_q.cpu().numpy(), q) and np.array_equal(s_ok.cpu().numpy().reshape(n), ok)
    assert np.array_equal(s_b.cpu().numpy(), base[True])
    r, rok = add_dev(api, pt, pt, False)
    assert np.array_equal(s_r.cpu().numpy(), r) and np.array_equal(s_rok.cpu().numpy().reshape(n), rok)
