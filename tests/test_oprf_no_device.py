"""The OPRF / VOPRF calls at the drop-in boundary without a device: the header, the ctypes table and curve25519_amd.oprf agree; every
wrapper checks its arguments before anything is asked of a device; every call fails with an error code and a message (EngineError
through curve25519_amd.oprf), there is no CPU result behind them and the output buffers stay as they were; n == 0 returns 0 all the
same.  With a GPU present the no-device half does not apply and only the argument rules are checked here (tests/test_gpu_oprf.py
holds the rest)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from curve25519_amd import _lib, api, oprf
from test_api_arguments import _claims_cuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ("ristretto255_OPRF_Blind", "ristretto255_OPRF_Finalize", "ristretto255_OPRF_BlindEvaluate", "ristretto255_VOPRF_BlindEvaluate",
         "ristretto255_VOPRF_VerifyProof")


def has_device():
    return _lib.load().c25519_amd_device_count() > 0


def test_header_table_and_module_name_the_same_calls():
    text = open(os.path.join(ROOT, "include", "curve25519_amd.h")).read()
    declared = set(re.findall(r"\b(ristretto255_V?OPRF_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == {s + f for s in STEMS for f in ("_batch", "_dev")} | {"ristretto255_VOPRF_scratch_bytes"}
    lib = _lib.load()
    for name in declared:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for s in STEMS:
        assert _lib.SIGNATURES[s + "_dev"] == _lib.SIGNATURES[s + "_batch"] + [C.c_void_p], s
    mine = {n for n, f in vars(oprf).items() if inspect.isfunction(f) and f.__module__ == oprf.__name__ and not n.startswith("_")}
    assert mine == set(STEMS) | {s + "_dev" for s in STEMS} | {"ristretto255_VOPRF_scratch_bytes"}
    assert not [n for n in vars(api) if "OPRF" in n], "the wrappers live in curve25519_amd/oprf.py"
    for macro, val in (("ristretto255_oprf_output_size", 64), ("ristretto255_voprf_proof_size", 64), ("ristretto255_voprf_max_rows", 65535)):
        assert re.search(rf"#define\s+{macro}\s+{val}\b", text)
    assert oprf.MAX_ROWS == 65535 and oprf.MAX_INPUT_SIZE == 65535


def test_scratch_bytes_is_the_header_formula():
    r4 = lambda x: (x + 3) // 4 * 4  # noqa: E731
    text = " ".join(re.sub(r"^\s*\*", " ", open(os.path.join(ROOT, "include", "curve25519_amd.h")).read(), flags=re.M).split())
    assert "4 * (8 * r4(10 n) + 2 * r4(n) + 32) bytes" in text
    for m, n in ((1, 1), (3, 5), (1, 65535), (4096, 1 << 20), (0, 0)):
        assert oprf.ristretto255_VOPRF_scratch_bytes(m, n) == 4 * (8 * r4(10 * n) + 2 * r4(n) + 32), (m, n)


def test_the_wrappers_check_shapes_and_modes():
    z = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    off = np.array([0, 2], np.uint64)
    bad = (
        lambda: oprf.ristretto255_OPRF_Blind(z(2, 4), z(2, 33)),                     # a row too wide
        lambda: oprf.ristretto255_OPRF_Blind(z(3, 4), z(2, 32)),                     # a row missing
        lambda: oprf.ristretto255_OPRF_Blind(z(2, 4), z(2, 32), mode=2),
        lambda: oprf.ristretto255_OPRF_Blind(z(2, 4), z(2, 32), mode=-1),
        lambda: oprf.ristretto255_OPRF_Blind(z(1, 65536), z(1, 32)),
        lambda: oprf.ristretto255_OPRF_Finalize(z(2, 4), z(2, 32), z(2, 31)),
        lambda: oprf.ristretto255_OPRF_Finalize(z(2, 4), z(2, 32), z(3, 32)),
        lambda: oprf.ristretto255_OPRF_Finalize(z(1, 65536), z(1, 32), z(1, 32)),
        lambda: oprf.ristretto255_OPRF_BlindEvaluate(z(2, 32), z(2, 32)),            # ONE key
        lambda: oprf.ristretto255_OPRF_BlindEvaluate(z(31), z(2, 32)),
        lambda: oprf.ristretto255_OPRF_BlindEvaluate(z(32), z(2, 64)),
        lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(1, 32), z(2, 32), np.array([0, 1, 2], np.uint64)),   # offsets for two requests
        lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(1, 64), z(2, 32), off),
        lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(1, 32), z(2, 32), np.array([0, 3], np.uint64)),      # past n
        lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(1, 32), z(2, 32), np.array([1, 2], np.uint64)),
        lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(2, 32), z(2, 32), np.array([0, 2, 2], np.uint64)),   # an empty request
        lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(2, 32), z(3, 32), np.array([0, 2, 1], np.uint64)),   # decreasing
        lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(1, 32), z(65536, 32), np.array([0, 65536], np.uint64)),
        lambda: oprf.ristretto255_VOPRF_VerifyProof(z(32), z(2, 32), z(3, 32), z(1, 64), off),
        lambda: oprf.ristretto255_VOPRF_VerifyProof(z(32), z(2, 32), z(2, 32), z(1, 63), off),
        lambda: oprf.ristretto255_VOPRF_VerifyProof(z(2, 32), z(2, 32), z(2, 32), z(1, 64), off),
    )
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {k} was accepted")


# the tensors of each _dev wrapper in the order of its parameters: (name, rows, width, dtype); width None: any (input_size).  M requests
# over N rows.  `counts`: the tensors whose row count the wrapper reads n or m from (one row more there is another call, not an error)
M, N = 2, 3
DEV_FORMS = {
    "ristretto255_OPRF_Blind_dev": ((("blinded", N, 32, "u8"), ("ok", N, 1, "i32"), ("input", N, None, "u8"), ("blind", N, 32, "u8")), ("blinded",)),
    "ristretto255_OPRF_Finalize_dev": ((("output", N, 64, "u8"), ("ok", N, 1, "i32"), ("input", N, None, "u8"), ("blind", N, 32, "u8"),
                                        ("evaluated", N, 32, "u8")), ("output",)),
    "ristretto255_OPRF_BlindEvaluate_dev": ((("evaluated", N, 32, "u8"), ("ok", N, 1, "i32"), ("skS", 1, 32, "u8"), ("blinded", N, 32, "u8")),
                                            ("evaluated",)),
    "ristretto255_VOPRF_BlindEvaluate_dev": ((("evaluated", N, 32, "u8"), ("proof", M, 64, "u8"), ("ok", N, 1, "i32"), ("req_ok", M, 1, "i32"),
                                             ("skS", 1, 32, "u8"), ("proof_rand", M, 32, "u8"), ("blinded", N, 32, "u8"), ("offsets", M + 1, 1, "i64")),
                                            ("evaluated", "proof_rand")),
    "ristretto255_VOPRF_VerifyProof_dev": ((("req_ok", M, 1, "i32"), ("pkS", 1, 32, "u8"), ("blinded", N, 32, "u8"), ("evaluated", N, 32, "u8"),
                                           ("proof", M, 64, "u8"), ("offsets", M + 1, 1, "i64")), ("blinded", "proof")),
}
WRONG_DTYPE = {"u8": "i32", "i32": "u8", "i64": "i32"}


def _dev_tensor(rows, width, dtype, cuda=True):
    import torch
    t = torch.zeros((rows, 5 if width is None else width), dtype={"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}[dtype])
    return torch.Tensor._make_subclass(_claims_cuda(), t) if cuda else t


def _dev_args(name, cuda=True, change=None):
    """the wrapper's tensors, all well formed but `change` = (argument, what): "dtype", "width" or "rows" """
    out = []
    for arg, rows, width, dtype in DEV_FORMS[name][0]:
        if change and change[0] == arg:
            dtype = WRONG_DTYPE[dtype] if change[1] == "dtype" else dtype
            width = width + 1 if change[1] == "width" else width
            rows = rows + 1 if change[1] == "rows" else rows
        out.append(_dev_tensor(rows, width, dtype, cuda))
    return out


@pytest.mark.parametrize("name", sorted(DEV_FORMS))
def test_the_device_forms_refuse_cpu_tensors(name):
    with pytest.raises(ValueError):
        getattr(oprf, name)(*_dev_args(name, cuda=False))
    for k in range(len(DEV_FORMS[name][0])):
        args = _dev_args(name)
        args[k] = None
        with pytest.raises(ValueError):
            getattr(oprf, name)(*args)


@pytest.mark.parametrize("name", sorted(DEV_FORMS))
def test_the_device_forms_refuse_a_wrong_dtype_width_or_row_count(name):
    """tensors that pass the wrappers' `is_cuda` test (tests/test_api_arguments.py's ClaimsCuda: host memory, nothing is launched), all
    well formed but one: the error names that argument, and the library is not reached"""
    specs, counts = DEV_FORMS[name]
    for arg, rows, width, dtype in specs:
        for what in ("dtype", "width", "rows"):
            if what == "width" and width is None:
                continue
            # one row more in a tensor the counts are read from makes every OTHER tensor the short one: still refused, under their names
            named = None if what == "rows" and arg in counts else rf"\b{arg}\b"
            with pytest.raises(ValueError, match=named):
                getattr(oprf, name)(*_dev_args(name, change=(arg, what)))


def test_the_device_forms_refuse_bad_modes_and_input_sizes():
    args = _dev_args("ristretto255_OPRF_Blind_dev")
    for mode in (2, -1, 7, None):
        with pytest.raises(ValueError, match="mode"):
            oprf.ristretto255_OPRF_Blind_dev(*args, mode)
    for name in ("ristretto255_OPRF_Blind_dev", "ristretto255_OPRF_Finalize_dev"):
        args = _dev_args(name)
        args[2] = _dev_tensor(N, 65536, "u8")
        with pytest.raises(ValueError, match="input_size"):
            getattr(oprf, name)(*args)


def test_the_library_refuses_bad_modes_sizes_and_offsets():
    lib = _lib.load()
    buf = np.full((4, 64), 0xA5, np.uint8)
    p = buf.ctypes.data
    for form, tail in (("_batch", ()), ("_dev", (None,))):
        assert getattr(lib, "ristretto255_OPRF_Blind" + form)(p, p, p, 8, p, 2, 1, *tail) != 0 and b"mode" in lib.c25519_amd_last_error()
        assert getattr(lib, "ristretto255_OPRF_Blind" + form)(p, p, p, 8, p, -1, 1, *tail) != 0 and b"mode" in lib.c25519_amd_last_error()
        assert getattr(lib, "ristretto255_OPRF_Blind" + form)(p, p, p, 65536, p, 0, 1, *tail) != 0 and b"65535" in lib.c25519_amd_last_error()
        assert getattr(lib, "ristretto255_OPRF_Finalize" + form)(p, p, p, 65536, p, p, 1, *tail) != 0 and b"65535" in lib.c25519_amd_last_error()
    for off in ([0, 2, 2, 3], [0, 2, 1, 3], [0, 1, 2, 4], [1, 2, 3, 3], [0, 1, 2, 2]):
        o = np.array(off, np.uint64)
        assert lib.ristretto255_VOPRF_BlindEvaluate_batch(p, p, p, p, p, p, p, o.ctypes.data, 3, 3) != 0, off
        assert b"offsets" in lib.c25519_amd_last_error() or b"request" in lib.c25519_amd_last_error(), off
        assert lib.ristretto255_VOPRF_VerifyProof_batch(p, p, p, p, p, o.ctypes.data, 3, 3) != 0, off
    o = np.array([0, 65536], np.uint64)
    assert lib.ristretto255_VOPRF_BlindEvaluate_batch(p, p, p, p, p, p, p, o.ctypes.data, 1, 65536) != 0 and b"65535" in lib.c25519_amd_last_error()
    assert (buf == 0xA5).all(), "a refused call writes nothing"


def test_a_null_pointer_is_an_argument_error():
    lib = _lib.load()
    buf = np.full((4, 64), 0xA5, np.uint8)
    p = buf.ctypes.data
    offsets = np.array([0, 1], np.uint64)                      # (held: .ctypes.data of a temporary dangles)
    off = offsets.ctypes.data
    for form, tail in (("_batch", ()), ("_dev", (None,))):
        for k in (0, 1, 2, 4):
            args = [p, p, p, 8, p, 0, 1]
            args[k] = None
            assert getattr(lib, "ristretto255_OPRF_Blind" + form)(*args, *tail) != 0 and b"null pointer" in lib.c25519_amd_last_error(), (form, k)
        for k in (0, 1, 2, 4, 5):
            args = [p, p, p, 8, p, p, 1]
            args[k] = None
            assert getattr(lib, "ristretto255_OPRF_Finalize" + form)(*args, *tail) != 0 and b"null pointer" in lib.c25519_amd_last_error(), (form, k)
        for k in range(4):
            args = [p, p, p, p, 1]
            args[k] = None
            assert getattr(lib, "ristretto255_OPRF_BlindEvaluate" + form)(*args, *tail) != 0 and b"null pointer" in lib.c25519_amd_last_error(), (form, k)
        for k in range(8):
            args = [p, p, p, p, p, p, p, off, 1, 1]
            args[k] = None
            assert getattr(lib, "ristretto255_VOPRF_BlindEvaluate" + form)(*args, *tail) != 0 and b"null pointer" in lib.c25519_amd_last_error(), (form, k)
        for k in range(6):
            args = [p, p, p, p, p, off, 1, 1]
            args[k] = None
            assert getattr(lib, "ristretto255_VOPRF_VerifyProof" + form)(*args, *tail) != 0 and b"null pointer" in lib.c25519_amd_last_error(), (form, k)
    assert (buf == 0xA5).all()


def test_a_call_of_nothing_returns_zero():
    lib = _lib.load()
    buf = np.full((1, 64), 0xA5, np.uint8)
    p = buf.ctypes.data
    offsets = np.array([0], np.uint64)
    off = offsets.ctypes.data
    for form, tail in (("_batch", ()), ("_dev", (None,))):
        assert getattr(lib, "ristretto255_OPRF_Blind" + form)(p, p, p, 8, p, 1, 0, *tail) == 0
        assert getattr(lib, "ristretto255_OPRF_Blind" + form)(p, p, None, 0, p, 0, 0, *tail) == 0, "input may be NULL when input_size is 0"
        assert getattr(lib, "ristretto255_OPRF_Finalize" + form)(p, p, p, 8, p, p, 0, *tail) == 0
        assert getattr(lib, "ristretto255_OPRF_BlindEvaluate" + form)(p, p, p, p, 0, *tail) == 0
        assert getattr(lib, "ristretto255_VOPRF_BlindEvaluate" + form)(p, p, p, p, p, p, p, off, 0, 0, *tail) == 0
        assert getattr(lib, "ristretto255_VOPRF_VerifyProof" + form)(p, p, p, p, p, off, 0, 0, *tail) == 0
    assert (buf == 0xA5).all()
    blinded, ok = oprf.ristretto255_OPRF_Blind(np.zeros((0, 7), np.uint8), np.zeros((0, 32), np.uint8))
    assert blinded.shape == (0, 32) and ok.shape == (0,)
    out, ok = oprf.ristretto255_OPRF_Finalize(np.zeros((0, 7), np.uint8), np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
    assert out.shape == (0, 64) and ok.shape == (0,)


def test_without_a_device_every_call_raises_and_leaves_no_result():
    if has_device():
        return
    z = lambda *s: np.ones(s, np.uint8)  # noqa: E731
    off = np.array([0, 2], np.uint64)
    for call in (lambda: oprf.ristretto255_OPRF_Blind(z(2, 5), z(2, 32), 1), lambda: oprf.ristretto255_OPRF_Blind(z(2, 0), z(2, 32)),
                 lambda: oprf.ristretto255_OPRF_Finalize(z(2, 5), z(2, 32), z(2, 32)), lambda: oprf.ristretto255_OPRF_BlindEvaluate(z(32), z(2, 32)),
                 lambda: oprf.ristretto255_VOPRF_BlindEvaluate(z(32), z(1, 32), z(2, 32), off),
                 lambda: oprf.ristretto255_VOPRF_VerifyProof(z(32), z(2, 32), z(2, 32), z(1, 64), off)):
        with pytest.raises(_lib.EngineError):
            call()
        assert _lib.load().c25519_amd_last_error() != b""
    lib = _lib.load()
    out, ok, src = np.full((3, 64), 0xA5, np.uint8), np.full(3, 0x5A5A5A5A, np.int32), np.ones((3, 64), np.uint8)
    offsets = np.array([0, 3], np.uint64)
    o, k, s, f = out.ctypes.data, ok.ctypes.data, src.ctypes.data, offsets.ctypes.data
    assert lib.ristretto255_OPRF_Blind_batch(o, k, s, 8, s, 0, 3) != 0 and lib.ristretto255_OPRF_Blind_dev(o, k, s, 8, s, 0, 3, None) != 0
    assert lib.ristretto255_OPRF_Finalize_batch(o, k, s, 8, s, s, 3) != 0 and lib.ristretto255_OPRF_Finalize_dev(o, k, s, 8, s, s, 3, None) != 0
    assert lib.ristretto255_OPRF_BlindEvaluate_batch(o, k, s, s, 3) != 0 and lib.ristretto255_OPRF_BlindEvaluate_dev(o, k, s, s, 3, None) != 0
    assert lib.ristretto255_VOPRF_BlindEvaluate_batch(o, o, k, k, s, s, s, f, 1, 3) != 0
    assert lib.ristretto255_VOPRF_BlindEvaluate_dev(o, o, k, k, s, s, s, f, 1, 3, None) != 0
    assert lib.ristretto255_VOPRF_VerifyProof_batch(k, s, s, s, s, f, 1, 3) != 0 and lib.ristretto255_VOPRF_VerifyProof_dev(k, s, s, s, s, f, 1, 3, None) != 0
    assert lib.c25519_amd_last_error() != b""
    assert (out == 0xA5).all() and (ok == 0x5A5A5A5A).all(), "a failed call writes no result"
    assert (src == 1).all()
