"""CPU tests of the multiscalar calls' lane functions (curve25519_amd/csrc/msm_sum.cuh: what ed25519_MultiScalarMult[_vartime]_* and
ristretto255_MultiScalarMult[_vartime]_* run on the device).  The device source is compiled by g++ against the C model of the gfx950
primitives (tests/host_emul/msm.cpp, tests/host_emul/build.py's open_lib) and judged byte for byte against the big-integer model
(tests/msm_model.py): the constant-time path at the chunk and pass boundaries, the bucket path -- a host counting sort between the
stages -- at the narrowest and the widest window, both groups."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import msm_model as model

vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int


class Emulated:
    def __init__(self, lib):
        self.lib = lib

    def _run(self, fn, group, sc, pt, m, *tail):
        n_groups = len(sc) // m
        sc, pt = np.ascontiguousarray(sc), np.ascontiguousarray(pt)
        before = (sc.copy(), pt.copy())
        q, ok = np.full((n_groups, 32), 0xA5, np.uint8), np.full(n_groups, -1, np.int32)
        fn(q.ctypes.data, ok.ctypes.data, sc.ctypes.data, pt.ctypes.data, m, n_groups, model.GROUPS.index(group), *tail)
        assert np.array_equal(sc, before[0]) and np.array_equal(pt, before[1])
        return q, ok

    def sum(self, group, sc, pt, m):
        return self._run(self.lib.emul_msm_sum, group, sc, pt, m)

    def bucket(self, group, sc, pt, m, c):
        return self._run(self.lib.emul_msm_bucket, group, sc, pt, m, c)


@pytest.fixture(scope="module")
def impl():
    lib = open_lib({"emul_msm_sum": ([vp, vp, vp, vp, sz, sz, ci], None), "emul_msm_bucket": ([vp, vp, vp, vp, sz, sz, ci, ci], None),
                    "emul_msm_chunk": ([], ci)}, "msm.cpp", "libc25519_emul_msm.so")
    yield Emulated(lib)
    assert_no_mad_overflow(lib)


def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])


def test_the_model_cuts_chunks_where_the_device_does(impl):
    assert impl.lib.emul_msm_chunk() == model.SUM_CHUNK == 64


@pytest.mark.parametrize("group", model.GROUPS)
@pytest.mark.parametrize("n_groups", (1, 3))
@pytest.mark.parametrize("m", (1, 2, 63, 64, 65, 4096, 4097))
def test_the_constant_time_path_at_chunk_and_pass_boundaries(impl, group, n_groups, m):
    sc, pt = model.case(group, n_groups, m, seed=11)
    _same(impl.sum(group, sc, pt, m), model.expected(group, sc, pt, m))


@pytest.mark.parametrize("group", model.GROUPS)
@pytest.mark.parametrize("c", (7, 13))
@pytest.mark.parametrize("m", model.BUCKET_M)
def test_the_bucket_path_at_the_narrowest_and_widest_window(impl, group, c, m):
    for n_groups in (1, 3):
        sc, pt = model.case(group, n_groups, m, seed=13)
        _same(impl.bucket(group, sc, pt, m, c), model.expected(group, sc, pt, m))


@pytest.mark.parametrize("group", model.GROUPS)
def test_equal_scalars_and_cancelling_groups_on_both_paths(impl, group):
    for kind, m in (("equal", 65), ("cancel", 130)):
        sc, pt = model.case(group, 2, m, seed=17, kind=kind)
        want = model.expected(group, sc, pt, m)
        if kind == "cancel":
            assert want[1].all() and all(bytes(r) == model.IDENTITY[group] for r in want[0])
        _same(impl.sum(group, sc, pt, m), want)
        for c in (7, 13):
            _same(impl.bucket(group, sc, pt, m, c), want)


@pytest.mark.parametrize("group", model.GROUPS)
def test_window_patterns_at_every_width(impl, group):
    """every scalar of the set (the edge values and each width's all-2^(c-1) and all-ones windows) meets every width"""
    m = 65
    sc, pt = model.case(group, 1, m, seed=19)
    want = model.expected(group, sc, pt, m)
    for c in model.WIDTHS:
        _same(impl.bucket(group, sc, pt, m, c), want)


@pytest.mark.parametrize("group", model.GROUPS)
def test_a_reject_zeroes_its_group_only_on_both_paths(impl, group):
    m, n_groups = 5, 3
    sc, pt = model.case(group, n_groups, m, seed=23)
    for which in ("non-decoding",) + (("non-canonical",) if group == "ristretto255" else ()):
        for row in (n_groups * m - 1, 0):
            bad = model.with_reject(group, pt, row, which)
            want = model.expected(group, sc, bad, m)
            assert want[1].sum() == n_groups - 1 and want[1][row // m] == 0
            _same(impl.sum(group, sc, bad, m), want)
            _same(impl.bucket(group, sc, bad, m, 10), want)
