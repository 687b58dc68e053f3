"""GPU suite for ed25519_MultiScalarMult[_vartime]_* and ristretto255_MultiScalarMult[_vartime]_* (include/curve25519_amd.h,
"multiscalar multiplication").  Every output must be the bytes of the big-integer model (tests/msm_model.py, held against the two
models it stands on by tests/test_msm_model.py): the default dispatch at the chunk and pass boundaries of the constant-time path, the
bucket path forced by MSM_BUCKET_MIN = 1 at every window width, plain and _vartime agreeing byte for byte, rejects that zero their own
group only, groups that cancel to the identity, _batch equal to _dev, and a captured graph that replays without allocating.
Byte-exact: no tolerance is involved."""
import functools

import numpy as np
import pytest

import msm_model as model
from curve25519_amd import _lib

pytestmark = pytest.mark.gpu

FILL, OK_FILL = 0xA5, 0x5A5A5A5A
STEM = {"ed25519": "ed25519_MultiScalarMult", "ristretto255": "ristretto255_MultiScalarMult"}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api as a, msm
    assert a.device_count() >= 1
    return msm


def to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(torch.device("cuda", 0))


def run_dev(api, group, sc, pt, m, vartime):
    """(q, ok) of the _dev form, after the inputs were seen unchanged and the guard rows behind the outputs untouched"""
    import torch
    n_groups = len(sc) // m
    d = torch.device("cuda", 0)
    q = torch.full((n_groups + 1, 32), FILL, dtype=torch.uint8, device=d)
    ok = torch.full((n_groups + 1, 1), OK_FILL, dtype=torch.int32, device=d)
    dsc, dpt = to_dev(sc), to_dev(pt)
    getattr(api, STEM[group] + ("_vartime" if vartime else "") + "_dev")(q[:-1], ok[:-1], dsc, dpt)
    torch.cuda.synchronize()
    assert np.array_equal(dsc.cpu().numpy(), sc) and np.array_equal(dpt.cpu().numpy(), pt), "inputs are never written"
    hq, hok = q.cpu().numpy(), ok.cpu().numpy().reshape(-1)
    assert (hq[-1] == FILL).all() and hok[-1] == OK_FILL, "nothing is written behind the last row"
    return hq[:-1], hok[:-1]


@functools.lru_cache(maxsize=None)
def _case(group, n_groups, m, seed=29, kind="mixed"):
    """(scalar, point, expected q, expected ok): computed once, shared by the tests that use the shape, never written"""
    sc, pt = model.case(group, n_groups, m, seed, kind)
    q, ok = model.expected(group, sc, pt, m)
    for a in (sc, pt, q, ok):
        a.setflags(write=False)
    return sc, pt, q, ok


def _check(got, q, ok):
    assert np.array_equal(got[1], ok)
    assert np.array_equal(got[0], q)


@pytest.mark.parametrize("group", model.GROUPS)
@pytest.mark.parametrize("shape", model.DEFAULT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_default_dispatch_matches_the_model_and_both_flavours_agree(api, group, shape):
    """at these sizes both flavours take the constant-time path: chunk boundaries 63 / 64 / 65, two passes at 4097, many small groups"""
    n_groups, m = shape
    sc, pt, q, ok = _case(group, n_groups, m)
    plain = run_dev(api, group, sc, pt, m, False)
    _check(plain, q, ok)
    _check(run_dev(api, group, sc, pt, m, True), *plain)


@pytest.mark.parametrize("group", model.GROUPS)
@pytest.mark.parametrize("width", model.WIDTHS + (-1,), ids=lambda w: "builtin" if w < 0 else f"c{w}")
def test_the_bucket_path_at_every_width(api, group, width):
    """MSM_BUCKET_MIN = 1 sends every _vartime call through the buckets; n_groups = 3 runs three groups over the same scratch, which
    must be re-zeroed in between; the scalar set holds the edge values and every width's window patterns"""
    with _lib.tunable("MSM_BUCKET_MIN", 1), _lib.tunable("MSM_WINDOW", width):
        for m in model.BUCKET_M:
            for n_groups in (1, 3):
                sc, pt, q, ok = _case(group, n_groups, m)
                _check(run_dev(api, group, sc, pt, m, True), q, ok)
    for m in (65, 300):                                    # ... and the plain call gives the same bytes
        sc, pt, q, ok = _case(group, 3, m)
        _check(run_dev(api, group, sc, pt, m, False), q, ok)


@pytest.mark.parametrize("group", model.GROUPS)
def test_the_built_in_threshold_between_the_paths(api, group):
    """with the tunables left alone a _vartime call of ONE group changes path at m = 2^10 (of more groups at 2^18): one row below and
    at the threshold, both flavours, the model's bytes"""
    assert _lib.load().c25519_amd_tunable_get(b"MSM_BUCKET_MIN") == -1 and _lib.load().c25519_amd_tunable_get(b"MSM_WINDOW") == -1
    for n_groups, m in ((1, 1023), (1, 1024), (2, 1024)):
        sc, pt, q, ok = _case(group, n_groups, m)
        for vartime in (False, True):
            _check(run_dev(api, group, sc, pt, m, vartime), q, ok)


@pytest.mark.parametrize("group", model.GROUPS)
def test_equal_scalars_and_the_mixed_order_point_on_both_paths(api, group):
    """one scalar everywhere: one long bucket list per window and the split top window; the Edwards pool holds a point of order 8 and a
    mixed-order point, on which only the mod-L reading of the scalar makes the two paths agree"""
    for m in (65, 300):
        sc, pt, q, ok = _case(group, 2, m, kind="equal")
        _check(run_dev(api, group, sc, pt, m, False), q, ok)
        for width in (7, 10, 13):
            with _lib.tunable("MSM_BUCKET_MIN", 1), _lib.tunable("MSM_WINDOW", width):
                _check(run_dev(api, group, sc, pt, m, True), q, ok)
    if group == "ed25519":
        mixed = np.frombuffer(model.pool(group)[0][11], np.uint8)
        sc = model._rows([model._le(v) for v in (model.L + 1, 2**256 - 1, 5, model.L - 1)])
        pt = np.stack([mixed] * 4)
        q, ok = model.expected(group, sc, pt, 2)
        _check(run_dev(api, group, sc, pt, 2, False), q, ok)
        with _lib.tunable("MSM_BUCKET_MIN", 1):
            _check(run_dev(api, group, sc, pt, 2, True), q, ok)


@pytest.mark.parametrize("group", model.GROUPS)
def test_a_reject_zeroes_its_group_only(api, group):
    """a point that does not decode as the last row of the last group, then as the first row of the first: that group alone gets
    ok = 0 and zero bytes, on both paths; the non-canonical ristretto255 encoding rejects as well"""
    n_groups, m = 3, 7
    sc, pt, _, _ = _case(group, n_groups, m)
    for which in ("non-decoding",) + (("non-canonical",) if group == "ristretto255" else ()):
        for row in (n_groups * m - 1, 0):
            bad = model.with_reject(group, pt, row, which)
            q, ok = model.expected(group, sc, bad, m)
            assert ok.tolist() == [0 if g == row // m else 1 for g in range(n_groups)] and not q[row // m].any()
            _check(run_dev(api, group, sc, bad, m, False), q, ok)
            with _lib.tunable("MSM_BUCKET_MIN", 1):
                _check(run_dev(api, group, sc, bad, m, True), q, ok)


@pytest.mark.parametrize("group", model.GROUPS)
def test_a_cancelling_group_is_the_identity(api, group):
    for m in (2, 130):
        sc, pt, q, ok = _case(group, 2, m, kind="cancel")
        assert ok.all() and all(bytes(r) == model.IDENTITY[group] for r in q)
        _check(run_dev(api, group, sc, pt, m, False), q, ok)
        with _lib.tunable("MSM_BUCKET_MIN", 1):
            _check(run_dev(api, group, sc, pt, m, True), q, ok)


@pytest.mark.parametrize("group", model.GROUPS)
def test_the_host_forms_give_the_device_forms_bytes(api, group):
    for n_groups, m in ((5, 7), (1, 300)):
        sc, pt, q, ok = _case(group, n_groups, m)
        for vartime in (False, True):
            got = getattr(api, STEM[group] + ("_vartime" if vartime else ""))(sc, pt, m)
            _check(got, q, ok)
            _check(run_dev(api, group, sc, pt, m, vartime), *got)
    with _lib.tunable("MSM_BUCKET_MIN", 1):
        sc, pt, q, ok = _case(group, 1, 300)
        _check(getattr(api, STEM[group] + "_vartime")(sc, pt, 300), q, ok)


def test_the_library_refuses_bad_sizes_on_the_device_too(api):
    import torch
    lib = _lib.load()
    buf = torch.full((4, 32), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    p = buf.data_ptr()
    for stem in STEM.values():
        for flavour in ("", "_vartime"):
            assert getattr(lib, stem + flavour + "_dev")(p, p, p, p, 0, 1, None) != 0
            assert getattr(lib, stem + flavour + "_dev")(p, p, p, p, (1 << 26) + 1, 1, None) != 0
            assert getattr(lib, stem + flavour + "_dev")(p, p, p, p, 4, 0, None) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()


@pytest.mark.parametrize("group", model.GROUPS)
@pytest.mark.parametrize("bucket", (False, True), ids=("sum", "bucket"))
def test_a_captured_graph_replays_and_allocates_nothing(api, group, bucket):
    """a _dev call on a side stream, captured and replayed twice, gives the same bytes; once the slab exists a call of the same shape
    takes no device memory"""
    import torch
    n_groups, m = 3, 130
    sc, pt, q, ok = _case(group, n_groups, m)
    d = torch.device("cuda", 0)
    dq = torch.full((n_groups, 32), FILL, dtype=torch.uint8, device=d)
    dok = torch.full((n_groups, 1), OK_FILL, dtype=torch.int32, device=d)
    dsc, dpt = to_dev(sc), to_dev(pt)
    call = getattr(api, STEM[group] + ("_vartime_dev" if bucket else "_dev"))
    side = torch.cuda.Stream()
    with _lib.tunable("MSM_BUCKET_MIN", 1 if bucket else -1):
        with torch.cuda.stream(side):
            call(dq, dok, dsc, dpt)
            side.synchronize()
            free = torch.cuda.mem_get_info()[0]
            call(dq, dok, dsc, dpt)
            side.synchronize()
            assert torch.cuda.mem_get_info()[0] == free, "a second call of the same shape allocates nothing"
        _check((dq.cpu().numpy(), dok.cpu().numpy().reshape(-1)), q, ok)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(dq, dok, dsc, dpt)
        for _ in range(2):
            dq.fill_(FILL)
            dok.fill_(OK_FILL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            _check((dq.cpu().numpy(), dok.cpu().numpy().reshape(-1)), q, ok)
