"""The two field representations the product did NOT choose (tools/ubench/field_forms.cuh: saturated 8 x 32 and
9 x 28.33-bit limbs) must be correct for the GPU A/B that times them (tools/ubench/field_ab.hip,
profiles/r02_field_ab.txt) to mean anything: field operations against Python big integers on the adversarial
patterns of tests/vectors.py, and a whole X25519 through each form's ladder step against the RFC 7748 / edge-key
vectors of the reference (tests/golden/kat.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from host_emul.build import open_lib
import vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))


@pytest.fixture(scope="module")
def forms():
    return open_lib({"forms_fe_op": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int],
                     "forms_x25519": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]},
                    "forms.cpp", "libc25519_forms.so", extra_include_dirs=[os.path.join(ROOT, "tools", "ubench")], mad_counter=False)


@pytest.mark.parametrize("form", [8, 9])
def test_alternative_field_forms_against_big_integers(forms, form):
    P = vectors.P
    pairs, a, b = vectors.field_cases()
    n = len(pairs)
    ops = {0: lambda x, y: x * y, 1: lambda x, y: x * x, 2: lambda x, y: x + y, 3: lambda x, y: x - y,
           4: lambda x, y: x + 121665 * y, 5: lambda x, y: pow(x, P - 2, P)}
    for op, f in ops.items():
        out = np.empty((n, 32), np.uint8)
        forms.forms_fe_op(out.ctypes.data, a.ctypes.data, b.ctypes.data, n, op, form)
        for i, (x, y) in enumerate(pairs):
            assert int.from_bytes(out[i].tobytes(), "little") == f(x, y) % P, (form, op, hex(x), hex(y))


@pytest.mark.parametrize("form", [8, 9])
def test_alternative_field_forms_run_x25519(forms, form):
    recs = KAT["x25519"]
    pk = np.concatenate([np.frombuffer(bytes.fromhex(r["pk"]), np.uint8).reshape(1, -1) for r in recs]).copy()
    sk = np.concatenate([np.frombuffer(bytes.fromhex(r["sk"]), np.uint8).reshape(1, -1) for r in recs]).copy()
    out = np.empty_like(pk)
    forms.forms_x25519(out.ctypes.data, pk.ctypes.data, sk.ctypes.data, len(recs), form)
    for i, r in enumerate(recs):
        assert out[i].tobytes().hex() == r["shared"], (form, r["name"])
