"""The multiscalar calls at the drop-in boundary without a device: the header, the ctypes table and curve25519_amd.msm name the same
eight entry points and the scratch function with the same signatures; the scratch function is callable without a device, does not
decrease in either size, and is what the two layouts of csrc/engine_msm.hip lease (recomputed here from their parts); the argument
rules hold before anything is asked of a device, and without one every call fails with an error and writes nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from curve25519_amd import _lib, api, msm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ("ed25519_MultiScalarMult", "ed25519_MultiScalarMult_vartime", "ristretto255_MultiScalarMult", "ristretto255_MultiScalarMult_vartime")
SCRATCH = "c25519_MultiScalarMult_scratch_bytes"


def has_device():
    return _lib.load().c25519_amd_device_count() > 0


def _header():
    text = open(os.path.join(ROOT, "include", "curve25519_amd.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_table_and_module_name_the_same_calls():
    text, code = _header()
    declared = set(re.findall(r"\b(\w*MultiScalarMult\w*)\s*\(", code))
    assert declared == {s + f for s in STEMS for f in ("_batch", "_dev")} | {SCRATCH}
    lib = _lib.load()
    for name in declared:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for s in STEMS:
        assert _lib.SIGNATURES[s + "_batch"] == [C.c_void_p] * 4 + [C.c_size_t] * 2, s
        assert _lib.SIGNATURES[s + "_dev"] == _lib.SIGNATURES[s + "_batch"] + [C.c_void_p], s
        proto = re.search(rf"\bint {s}_dev\(([^)]*)\)", code).group(1)
        assert [p.strip().split()[-1].lstrip("*") for p in proto.split(",")] == ["q", "ok", "scalar", "point", "m", "n_groups", "stream"]
        assert callable(getattr(msm, s)) and callable(getattr(msm, s + "_dev"))
        assert not hasattr(api, s), "the wrappers live in curve25519_amd/msm.py"
    assert _lib.SIGNATURES[SCRATCH] == [C.c_size_t, C.c_size_t, C.c_int] and _lib._RESTYPE[SCRATCH] is C.c_size_t
    assert re.search(r"\bsize_t c25519_MultiScalarMult_scratch_bytes\(size_t m, size_t n_groups, int vartime\);", code)
    assert re.search(r"#define\s+c25519_multiscalar_max_m\s+67108864\b", text) and msm.MULTISCALAR_MAX_M == 1 << 26
    for word in ("REDUCED MOD L", "THEIR RUNNING TIME AND THEIR MEMORY ACCESSES DEPEND ON THE SCALARS", "never cut across"):
        assert word in " ".join(re.sub(r"^\s*\*", " ", text, flags=re.M).split()), word
    for name in ("MSM_BUCKET_MIN", "MSM_WINDOW"):
        assert lib.c25519_amd_tunable_get(name.encode()) == -1, name


def r4(x):
    return (x + 3) // 4 * 4


def sum_layout_bytes(m, g):
    """msm_sum_layout: the rows' points (40 words each), one pass's output, both flag arrays, the Edwards finish's projective part"""
    after = (m + 63) // 64 * g if m > 1 else 0
    return 4 * (40 * m * g + 40 * after + r4(m * g) + r4(after) + 4 * r4(10 * g) + r4(g))


def bucket_layout_bytes(m, c):
    """msm_bucket_layout for one group: rows, bucket and window sums, scalars, entries, then flags, counts, cursor and the reject word"""
    wa = (253 + 2 + c - 1) // c
    K = wa << (c - 1)
    return 4 * (32 * m + 40 * K + 40 * wa + 8 * m + r4(m * wa) + r4(m) + 2 * K + 4)


def test_scratch_bytes_is_what_the_layouts_lease_and_needs_no_device():
    f = msm.c25519_MultiScalarMult_scratch_bytes
    shapes = ((1, 1), (2, 1), (1, 3), (63, 2), (64, 2), (65, 2), (4097, 2), (300, 1), (1 << 16, 1), (1 << 20, 1), (2, 1 << 19))
    for m, g in shapes:
        assert f(m, g, False) == sum_layout_bytes(m, g), (m, g)
    with _lib.tunable("MSM_BUCKET_MIN", 0):
        for m, g in shapes:
            assert f(m, g, True) == sum_layout_bytes(m, g), (m, g)
    with _lib.tunable("MSM_BUCKET_MIN", 1):
        for m, g in shapes:
            assert f(m, g, False) == sum_layout_bytes(m, g), "the plain call never takes the bucket path"
            assert f(m, g, True) == bucket_layout_bytes(m, 10 if m < 1 << 14 else 11 if m < 1 << 17 else 12), (m, g)
            for c in range(7, 14):
                with _lib.tunable("MSM_WINDOW", c):
                    assert f(m, g, True) == bucket_layout_bytes(m, c), (m, g, c)
    for g, lg in ((1, 10), (2, 18), (31, 18)):             # the built-in MSM_BUCKET_MIN: 2^10 for one group, 2^18 for more
        assert f(1 << lg, g, True) == bucket_layout_bytes(1 << lg, 10 if lg < 14 else 12), (g, lg)
        assert f((1 << lg) - 1, g, True) == sum_layout_bytes((1 << lg) - 1, g), (g, lg)
    assert f(0, 1, False) == 0 and f(1, 0, False) == 0 and f((1 << 26) + 1, 1, True) == 0 and f(1 << 26, 64, False) == 0


def test_scratch_bytes_does_not_decrease_in_either_size():
    """on either path: the plain call, and the _vartime call with the bucket path off and forced (one group's scratch serves every
    group there, so n_groups does not enter); across MSM_BUCKET_MIN the _vartime call changes path, which is not what is compared"""
    f = msm.c25519_MultiScalarMult_scratch_bytes
    sizes = (1, 2, 3, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65535, 65536, 65537, 1 << 20)
    for vartime, bucket_min in ((False, -1), (True, 0), (True, 1)):
        with _lib.tunable("MSM_BUCKET_MIN", bucket_min):
            for g in (1, 2, 3, 31):
                got = [f(m, g, vartime) for m in sizes]
                assert all(a <= b for a, b in zip(got, got[1:])) and got[0] > 0, (vartime, bucket_min, g)
            for m in sizes[:-1]:
                got = [f(m, g, vartime) for g in (1, 2, 3, 31, 32)]
                assert all(a <= b for a, b in zip(got, got[1:])), (vartime, bucket_min, m)


def test_the_wrappers_check_shapes():
    z = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    for s in STEMS:
        f = getattr(msm, s)
        for call in (lambda: f(z(4, 32), z(4, 31), 2), lambda: f(z(4, 32), z(3, 32), 2), lambda: f(z(5, 32), z(5, 32), 2),
                     lambda: f(z(4, 32), z(4, 32), 0), lambda: f(z(4, 32), z(4, 32), (1 << 26) + 1)):
            with pytest.raises(ValueError):
                call()
        for args in ((None, None, None, None), (z(2, 32), z(2, 1), z(4, 32), z(4, 32))):
            with pytest.raises(ValueError):
                getattr(msm, s + "_dev")(*args)


def test_the_library_checks_its_arguments_before_it_needs_a_device():
    lib = _lib.load()
    buf = np.full((8, 32), 0xA5, np.uint8)
    p = buf.ctypes.data
    for s in STEMS:
        for form, tail in (("_batch", ()), ("_dev", (None,))):
            fn = getattr(lib, s + form)
            for k in range(4):
                args = [p, p, p, p, 2, 2]
                args[k] = None
                assert fn(*args, *tail) != 0 and b"null pointer" in lib.c25519_amd_last_error(), (s, form, k)
            assert fn(p, p, p, p, 0, 2, *tail) != 0 and b"m must be" in lib.c25519_amd_last_error(), (s, form)
            assert fn(p, p, p, p, 0, 0, *tail) != 0, "m = 0 is an error whatever n_groups is"
            assert fn(p, p, p, p, (1 << 26) + 1, 1, *tail) != 0 and b"2^26" in lib.c25519_amd_last_error(), (s, form)
            assert fn(p, p, p, p, 1 << 26, 33, *tail) != 0 and b"2^31" in lib.c25519_amd_last_error(), (s, form)
            assert fn(p, p, p, p, 2, 0, *tail) == 0, "n_groups = 0 returns 0"
    assert (buf == 0xA5).all(), "a refused call writes nothing"


def test_without_a_device_every_call_raises_and_leaves_no_result():
    if has_device():
        return
    lib = _lib.load()
    one = np.ones((4, 32), np.uint8)
    for s in STEMS:
        with pytest.raises(_lib.EngineError):
            getattr(msm, s)(one, one, 2)
        assert lib.c25519_amd_last_error() != b""
        q, ok = np.full((2, 32), 0xA5, np.uint8), np.full(2, 0x5A5A5A5A, np.int32)
        assert getattr(lib, s + "_batch")(q.ctypes.data, ok.ctypes.data, one.ctypes.data, one.ctypes.data, 2, 2) != 0
        assert getattr(lib, s + "_dev")(q.ctypes.data, ok.ctypes.data, one.ctypes.data, one.ctypes.data, 2, 2, None) != 0
        assert (q == 0xA5).all() and (ok == 0x5A5A5A5A).all() and (one == 1).all(), "a failed call writes no result"
