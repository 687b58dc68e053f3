"""GPU suite (MI355X): ristretto255_IsValidPoint_*, ristretto255_FromHash_*, ristretto255_ScalarMult_*, ristretto255_ScalarMultBase_*,
ristretto255_PointAdd_* and ristretto255_PointSub_*.  Every output must be the bytes of the big-integer model of RFC 9496
(tests/ristretto_model.py, pinned to the RFC's vectors by tests/test_ristretto_model.py) on the case set the CPU tests share, at
every window width of the variable-base walk, at every size and in both forms; the calls must agree with each other, write every
row, and leave the caller's scalar bytes alone."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import ristretto_model as model
from curve25519_amd import _lib
from vectors import L

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 4097)      # the block and wave edges of a one-lane-per-element kernel
FILL = 0xA5
ZERO32 = bytes(32)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def cases():
    """the shared case set with the model's answers, computed once: 250 scalar / point pairs, the points and hashes on their own,
    the addition pairs"""
    sc, pt, labels = model.case_set()
    pts, plabels = model.points()
    h = model.hashes()
    ap, aq, names = model.add_cases()
    reject = np.flatnonzero(np.array(labels) != "valid")
    return dict(sc=sc, pt=pt, labels=labels, mult=model.expected_scalarmult(sc, pt), base=model.expected_base(sc), pts=pts,
                plabels=plabels, valid=model.expected_valid(pts), h=h, mapped=model.expected_from_hash(h), ap=ap, aq=aq, names=names,
                added={sub: model.expected_add(ap, aq, sub) for sub in (False, True)}, reject=reject)


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


def scalarmult_dev(api, sc, pt):
    import torch
    n = len(sc)
    d_sc, d_q, d_ok = to_dev(sc), filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
    api.ristretto255_ScalarMult_dev(d_q, d_ok, d_sc, to_dev(pt))
    torch.cuda.synchronize()
    assert np.array_equal(d_sc.cpu().numpy(), sc), "the scalar bytes are not written"
    return d_q.cpu().numpy(), d_ok.cpu().numpy().reshape(n)


def base_dev(api, sc):
    import torch
    d_sc, d_q = to_dev(sc), filled((len(sc), 32), torch.uint8)
    api.ristretto255_ScalarMultBase_dev(d_q, d_sc)
    torch.cuda.synchronize()
    assert np.array_equal(d_sc.cpu().numpy(), sc), "the scalar bytes are not written"
    return d_q.cpu().numpy()


def add_dev(api, p, q, sub):
    import torch
    n = len(p)
    d_r, d_ok = filled((n, 32), torch.uint8), filled((n, 4), torch.int32)
    (api.ristretto255_PointSub_dev if sub else api.ristretto255_PointAdd_dev)(d_r, d_ok, to_dev(p), to_dev(q))
    torch.cuda.synchronize()
    return d_r.cpu().numpy(), d_ok.cpu().numpy().reshape(n)


def valid_dev(api, pt):
    import torch
    d_ok = filled((len(pt), 4), torch.int32)
    api.ristretto255_IsValidPoint_dev(d_ok, to_dev(pt))
    torch.cuda.synchronize()
    return d_ok.cpu().numpy().reshape(len(pt))


def from_hash_dev(api, h):
    import torch
    d_h, d_p = to_dev(h), filled((len(h), 32), torch.uint8)
    api.ristretto255_FromHash_dev(d_p, d_h)
    torch.cuda.synchronize()
    assert np.array_equal(d_h.cpu().numpy(), h)
    return d_p.cpu().numpy()


def rows_differ(got, want):
    return np.flatnonzero((got != want).any(axis=1))


def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def value(row):
    return int.from_bytes(row.tobytes(), "little")


@pytest.mark.parametrize("w", model.WINDOWS)
def test_case_set(api, cases, w):
    """the whole case set through _dev and _batch at window width w: the model's bytes and ok in both forms"""
    sc, pt, labels = cases["sc"], cases["pt"], cases["labels"]
    q, ok = cases["mult"]
    with _lib.tunable("SCALARMULT_WINDOW", w):
        got, got_ok = scalarmult_dev(api, sc, pt)
        assert np.array_equal(got_ok, ok), [(i, labels[i]) for i in np.flatnonzero(got_ok != ok)][:8]
        bad = rows_differ(got, q)
        assert not len(bad), [(int(i), labels[i], sc[i].tobytes().hex(), got[i].tobytes().hex(), q[i].tobytes().hex()) for i in bad][:4]
        before = sc.copy()
        host, host_ok = api.ristretto255_ScalarMult(sc, pt)
        assert np.array_equal(host, q) and np.array_equal(host_ok, ok) and np.array_equal(sc, before)
        assert not got[ok == 0].any() and set(np.unique(got_ok)) == {0, 1}
    assert _lib.load().c25519_amd_tunable_get(b"SCALARMULT_WINDOW") == -1, "the tunable is restored"


def test_case_set_valid_hash_base_add_sub(api, cases):
    pts, plabels, valid = cases["pts"], cases["plabels"], cases["valid"]
    got = valid_dev(api, pts)
    assert np.array_equal(got, valid), [(i, plabels[i]) for i in np.flatnonzero(got != valid)][:8]
    assert np.array_equal(api.ristretto255_IsValidPoint(pts), valid)
    h, mapped = cases["h"], cases["mapped"]
    got = from_hash_dev(api, h)
    bad = rows_differ(got, mapped)
    assert not len(bad), [(int(i), h[i].tobytes().hex(), got[i].tobytes().hex(), mapped[i].tobytes().hex()) for i in bad][:4]
    assert np.array_equal(api.ristretto255_FromHash(h), mapped)
    sc, base = cases["sc"], cases["base"]
    assert not len(rows_differ(base_dev(api, sc), base))
    before = sc.copy()
    assert np.array_equal(api.ristretto255_ScalarMultBase(sc), base) and np.array_equal(sc, before)
    p, q, names = cases["ap"], cases["aq"], cases["names"]
    for sub in (False, True):
        r, ok = cases["added"][sub]
        got, got_ok = add_dev(api, p, q, sub)
        assert np.array_equal(got_ok, ok), [(i, names[i]) for i in np.flatnonzero(got_ok != ok)][:8]
        bad = rows_differ(got, r)
        assert not len(bad), [(int(i), names[i], got[i].tobytes().hex(), r[i].tobytes().hex()) for i in bad][:4]
        host, host_ok = (api.ristretto255_PointSub if sub else api.ristretto255_PointAdd)(p, q)
        assert np.array_equal(host, r) and np.array_equal(host_ok, ok)
        assert not got[ok == 0].any()


def tiled(cases, n):
    """n rows of the pool in a seeded permutation, rejected points in the first and last rows and on both sides of every 64-lane
    boundary"""
    sc, reject = cases["sc"], cases["reject"]
    rng = np.random.default_rng(0x6B + n)
    idx = np.concatenate([rng.permutation(len(sc)) for _ in range(n // len(sc) + 1)])[:n]
    at = sorted({0, n - 1} | {p for b in range(64, n, 64) for p in (b - 1, b)})
    if n > 2:
        idx[at] = reject[(np.arange(len(at)) * 7 + n) % len(reject)]
    return idx


@pytest.mark.parametrize("n", SIZES)
def test_sizes(api, cases, n):
    """every call at n elements, the walk at every width, rows drawn from the case set: every row of buffers pre-filled with 0xA5
    is the model's, in both forms"""
    sc, pt = cases["sc"], cases["pt"]
    q, ok = cases["mult"]
    idx = tiled(cases, n)
    s, p = sc[idx], pt[idx]
    for w in model.WINDOWS:
        with _lib.tunable("SCALARMULT_WINDOW", w):
            got, got_ok = scalarmult_dev(api, s, p)
            assert np.array_equal(got_ok, ok[idx]) and not len(rows_differ(got, q[idx])), w
    host, host_ok = api.ristretto255_ScalarMult(s, p)
    assert np.array_equal(host_ok, ok[idx]) and np.array_equal(host, q[idx])
    assert np.array_equal(base_dev(api, s), cases["base"][idx])
    assert np.array_equal(api.ristretto255_ScalarMultBase(s), cases["base"][idx])
    rng = np.random.default_rng(0xADE + n)
    j = rng.integers(0, len(cases["ap"]), n)
    for sub in (False, True):
        r, rok = cases["added"][sub]
        got, got_ok = add_dev(api, cases["ap"][j], cases["aq"][j], sub)
        assert np.array_equal(got_ok, rok[j]) and np.array_equal(got, r[j])
        host, host_ok = (api.ristretto255_PointSub if sub else api.ristretto255_PointAdd)(cases["ap"][j], cases["aq"][j])
        assert np.array_equal(host_ok, rok[j]) and np.array_equal(host, r[j])
    k = rng.integers(0, len(cases["pts"]), n)
    assert np.array_equal(valid_dev(api, cases["pts"][k]), cases["valid"][k])
    assert np.array_equal(api.ristretto255_IsValidPoint(cases["pts"][k]), cases["valid"][k])
    m = rng.integers(0, len(cases["h"]), n)
    assert np.array_equal(from_hash_dev(api, cases["h"][m]), cases["mapped"][m])
    assert np.array_equal(api.ristretto255_FromHash(cases["h"][m]), cases["mapped"][m])


def test_identities_between_calls(api, cases):
    """ScalarMultBase(e) == ScalarMult(e, enc(B)); PointAdd([a]B, [b]B) == ScalarMultBase(a + b mod L); PointSub(P, P) is zero bytes
    with ok = 1; the scalars L, 0 and 2^255 - 1; every FromHash output is valid; a rejected row leaves its neighbours untouched"""
    rng = np.random.default_rng(0x9496)
    n = 96
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    base_pt = np.tile(np.frombuffer(model.BASE, np.uint8), (n, 1))
    want = api.ristretto255_ScalarMultBase(sc)
    for i in range(0, n, 12):
        assert want[i].tobytes() == model.scalarmult_base(sc[i].tobytes()), i
    for w in model.WINDOWS:
        with _lib.tunable("SCALARMULT_WINDOW", w):
            q, ok = api.ristretto255_ScalarMult(sc, base_pt)
            assert ok.all() and np.array_equal(q, want), w
    a, b = sc[: n // 2], sc[n // 2:]
    mask = (1 << 255) - 1
    total = np.stack([le32(((value(x) & mask) + (value(y) & mask)) % L) for x, y in zip(a, b)])
    r, ok = api.ristretto255_PointAdd(want[: n // 2], want[n // 2:])
    assert ok.all() and np.array_equal(r, api.ristretto255_ScalarMultBase(total))
    diff = np.stack([le32(((value(x) & mask) - (value(y) & mask)) % L) for x, y in zip(a, b)])
    r, ok = api.ristretto255_PointSub(want[: n // 2], want[n // 2:])
    assert ok.all() and np.array_equal(r, api.ristretto255_ScalarMultBase(diff))
    r, ok = api.ristretto255_PointSub(want, want)
    assert ok.all() and not r.any(), "P - P is the identity: zero bytes with ok = 1"
    # L and 0 give the identity (zero bytes, ok = 1), 2^255 - 1 is e itself, bit 255 is ignored
    h = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    pts = api.ristretto255_FromHash(h)
    assert (api.ristretto255_IsValidPoint(pts) == 1).all(), "every FromHash output decodes"
    for i in range(0, n, 16):
        assert pts[i].tobytes() == model.from_hash(h[i].tobytes()), i
    for v in (L, 0):
        q, ok = api.ristretto255_ScalarMult(np.tile(le32(v), (n, 1)), pts)
        assert ok.all() and not q.any(), v
        assert not api.ristretto255_ScalarMultBase(le32(v).reshape(1, 32)).any()
    top = (1 << 255) - 1
    q, ok = api.ristretto255_ScalarMult(np.tile(le32(top), (n, 1)), pts)
    q2, ok2 = api.ristretto255_ScalarMult(np.tile(le32(top % L), (n, 1)), pts)
    q3, ok3 = api.ristretto255_ScalarMult(np.tile(le32((1 << 256) - 1), (n, 1)), pts)
    assert ok.all() and ok2.all() and ok3.all() and np.array_equal(q, q2) and np.array_equal(q, q3) and q.any(axis=1).all()
    assert q[0].tobytes() == model.scalarmult(le32(top).tobytes(), pts[0].tobytes())[0]
    assert np.array_equal(api.ristretto255_ScalarMultBase(le32(top).reshape(1, 32)), api.ristretto255_ScalarMultBase(le32(top % L).reshape(1, 32)))
    # one rejected row among valid ones, at a wave edge and inside a wave
    clean_q, clean_ok = api.ristretto255_ScalarMult(sc, pts)
    for at, (bad, _) in zip((0, 31, 63, 64, 95), model.FIXED_REJECTS):
        mixed = pts.copy()
        mixed[at] = np.frombuffer(bad, np.uint8)
        got, got_ok = scalarmult_dev(api, sc, mixed)
        keep = np.arange(n) != at
        assert got_ok[at] == 0 and not got[at].any()
        assert np.array_equal(got[keep], clean_q[keep]) and (got_ok[keep] == 1).all()
        r, rok = add_dev(api, mixed, pts, False)
        r2, rok2 = add_dev(api, pts, mixed, True)
        assert rok[at] == 0 and not r[at].any() and (rok[keep] == 1).all() and rok2[at] == 0 and not r2[at].any()
        assert valid_dev(api, mixed)[at] == 0 and valid_dev(api, mixed)[keep].all()


def test_oprf_round_trip(api):
    """ScalarMult(1/r, ScalarMult(k, ScalarMult(r, FromHash(h)))) == ScalarMult(k, FromHash(h)) for k, r nonzero mod L, 1/r mod L
    computed here"""
    rng = np.random.default_rng(0x0F8F)
    n = 257
    h = np.stack([np.frombuffer(hashlib.sha512(b"input %d" % i).digest(), np.uint8) for i in range(n)])
    ks, rs = [], []
    while len(ks) < n:
        k, r = (int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % L for _ in range(2))
        if k and r:
            ks.append(k); rs.append(r)
    k = np.stack([le32(v) for v in ks])
    r = np.stack([le32(v) for v in rs])
    r_inv = np.stack([le32(pow(v, L - 2, L)) for v in rs])
    p = api.ristretto255_FromHash(h)
    blinded, ok1 = api.ristretto255_ScalarMult(r, p)
    evaluated, ok2 = api.ristretto255_ScalarMult(k, blinded)
    unblinded, ok3 = api.ristretto255_ScalarMult(r_inv, evaluated)
    direct, ok4 = api.ristretto255_ScalarMult(k, p)
    assert ok1.all() and ok2.all() and ok3.all() and ok4.all()
    assert np.array_equal(unblinded, direct) and direct.any(axis=1).all()
    assert len(rows_differ(blinded, p)) == n and len({x.tobytes() for x in direct}) == n


def test_arguments(api, cases):
    """n == 0 returns 0 and writes nothing, a null or misaligned pointer is an argument error, a call on another stream gives the
    same bytes"""
    import torch
    sc, pt = cases["sc"], cases["pt"]
    h = cases["h"]
    L_ = _lib.load()
    d_sc, d_pt, d_h = to_dev(sc), to_dev(pt), to_dev(h)
    d_q, d_ok = filled((4, 32), torch.uint8), filled((4, 4), torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    h_q, h_ok = np.full((4, 32), FILL, np.uint8), np.full(4, 0x25A5A5A5, np.int32)
    calls = {                                                  # name: (device arguments, host arguments)
        "ristretto255_ScalarMult": ([p(d_q), p(d_ok), p(d_sc), p(d_pt)], [hp(h_q), hp(h_ok), hp(sc), hp(pt)]),
        "ristretto255_PointAdd": ([p(d_q), p(d_ok), p(d_pt), p(d_pt)], [hp(h_q), hp(h_ok), hp(pt), hp(pt)]),
        "ristretto255_PointSub": ([p(d_q), p(d_ok), p(d_pt), p(d_pt)], [hp(h_q), hp(h_ok), hp(pt), hp(pt)]),
        "ristretto255_ScalarMultBase": ([p(d_q), p(d_sc)], [hp(h_q), hp(sc)]),
        "ristretto255_FromHash": ([p(d_q), p(d_h)], [hp(h_q), hp(h)]),
        "ristretto255_IsValidPoint": ([p(d_ok), p(d_pt)], [hp(h_ok), hp(pt)]),
    }
    refused = []
    for name, (dev_args, host_args) in calls.items():
        assert getattr(L_, name + "_dev")(*dev_args, 0, None) == 0
        assert getattr(L_, name + "_batch")(*host_args, 0) == 0
        for k in range(len(dev_args)):
            refused.append(getattr(L_, name + "_dev")(*[None if i == k else a for i, a in enumerate(dev_args)], 4, None))
            assert b"null pointer" in L_.c25519_amd_last_error()
            refused.append(getattr(L_, name + "_batch")(*[None if i == k else a for i, a in enumerate(host_args)], 4))
            assert b"null pointer" in L_.c25519_amd_last_error()
    assert all(rc != 0 for rc in refused)
    off = C.c_void_p(d_sc.data_ptr() + 8)
    assert L_.ristretto255_ScalarMult_dev(p(d_q), p(d_ok), off, p(d_pt), 4, None) != 0, "a misaligned device pointer is refused"
    assert L_.ristretto255_ScalarMultBase_dev(p(d_q), off, 4, None) != 0
    assert L_.ristretto255_FromHash_dev(p(d_q), off, 4, None) != 0
    torch.cuda.synchronize()
    for t in (d_q, d_ok):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all(), "a refused call and a call of nothing write nothing"
    assert (h_q == FILL).all() and (h_ok == 0x25A5A5A5).all()
    assert np.array_equal(d_sc.cpu().numpy(), sc)
    side = torch.cuda.Stream(device=dev())
    n = len(sc)
    with torch.cuda.stream(side):
        s_q, s_ok, s_b = filled((n, 32), torch.uint8), filled((n, 4), torch.int32), filled((n, 32), torch.uint8)
        s_p = filled((len(h), 32), torch.uint8)
        api.ristretto255_ScalarMult_dev(s_q, s_ok, d_sc, d_pt)
        api.ristretto255_ScalarMultBase_dev(s_b, d_sc)
        api.ristretto255_FromHash_dev(s_p, d_h)
    side.synchronize()
    q, ok = cases["mult"]
    assert np.array_equal(s_q.cpu().numpy(), q) and np.array_equal(s_ok.cpu().numpy().reshape(n), ok)
    assert np.array_equal(s_b.cpu().numpy(), cases["base"]) and np.array_equal(s_p.cpu().numpy(), cases["mapped"])
