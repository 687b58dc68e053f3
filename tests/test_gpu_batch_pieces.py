"""GPU suite (MI355X): the host-pointer (*_batch) calls of the key, group, ristretto255, scalar, hashing, VRF and indexed-signing
families cut into pipeline pieces (csrc/host_pipeline.hpp run_batch).  Their own suites stop below 2^17 rows, where a call is one
piece: the count equals n and the offsets start at 0, so a wrapper that hands a piece the call's n, lists an array with the wrong
width or shares scratch between the two kernel lanes passes them.  Here every call runs through the C ABI on buffers the test
owns -- outputs of n + 1 rows of 0xA5 bytes -- as 65 536 + 65 536 + 3 rows under the default knobs, as 23 pieces of 5632 rows and one
of 1537 in a child process (three times the buffer sets, twelve turns of each kernel stream, three stagers and two drainers), and
once at the staging cap.  Every row must be the cycled expectation of the big-integer models or the oracle (tests/piece_cases.py;
the rows and why their period hides no misplaced piece: tests/test_piece_cases.py), the guard row must survive and the inputs stay
as they were.  Byte-exact: no tolerance is involved."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import piece_cases as pc
from curve25519_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the child: the period rows and their expectations arrive in a small .npz, are cycled to n rows there, and one JSON line comes back
CHILD = (
    "import json, sys; sys.path[:0] = [%r, %r]\n"
    "import numpy as np\n"
    "import piece_cases as pc\n"
    "from curve25519_amd import _lib\n"
    "arrays = dict(np.load(sys.argv[1]))\n"
    "lib = _lib.load()\n"
    "if sys.argv[2] == 'cap':\n"
    "    out = [pc.run_call(lib, pc.CAP_CALL, arrays, pc.CAP_N)]\n"
    "else:\n"
    "    out = pc.run_family(lib, sys.argv[2], arrays, pc.CUT_N, small_after=True)\n"
    "print(json.dumps(out))\n") % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    return _lib.load()


@pytest.fixture(scope="module", params=pc.FAMILIES)
def family(request):
    """one family a test; its rows are modelled here, once for both tests, so that --durations shows the models' time (setup) apart
    from the calls' (call)"""
    pc.family_rows(request.param)
    return request.param


def in_a_child(what, arrays, knobs):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rows.npz")
        np.savez(path, **arrays)
        assert os.path.getsize(path) < 4 << 20, "only the period rows travel"
        p = subprocess.run([sys.executable, "-c", CHILD, path, what], capture_output=True, text=True, timeout=240,
                           env={**os.environ, **knobs})
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_default_pieces(lib, family):
    """DEFAULT_N rows under the default knobs: two pieces of 65 536 rows on the two kernel streams and a tail of three rows that is a
    piece of its own; the scalar calls also with the output over each of their 32-byte inputs"""
    arrays = pc.family_rows(family)
    results = pc.run_family(lib, family, arrays, pc.DEFAULT_N)
    assert len(results) == len(pc.CALLS[family]) + len(pc.in_place_variants(family))
    assert all(r["n"] == pc.DEFAULT_N and r["chunk"] == 65536 for r in results)
    assert not pc.failures(results), pc.failures(results)[:3]


def test_many_pieces(family):
    """CUT_N rows in a fresh process under CUT_KNOBS (the knobs are read once per process): 24 pieces over 8 buffer sets; for the two
    families that lease scratch from the lanes' slabs, a call of 4097 rows right behind them"""
    arrays = pc.family_rows(family)
    results = in_a_child(family, arrays, pc.CUT_KNOBS)
    cut = [r for r in results if r["n"] == pc.CUT_N]
    assert len(cut) == len(pc.CALLS[family]) + len(pc.in_place_variants(family)) and all(r["chunk"] == 5632 for r in cut)
    small = [r for r in results if r["n"] == pc.SMALL_N]
    assert len(small) == len(pc.SMALL_AFTER.get(family, [])) == len(results) - len(cut) and all(r["chunk"] == pc.SMALL_N for r in small)
    assert not pc.failures(results), pc.failures(results)[:3]


def test_cap_cuts_a_call_below_the_piece_threshold():
    """The staging cap (256 MiB per buffer set) cuts a call that the row count would not: ed25519_HashToScalar_batch over CAP_N = 4101
    messages of CAP_MSG_SIZE = 65 505 bytes is a piece of 4096 rows and one of 5.  The 270 MB of messages are what reaching the cap
    takes -- this is the smallest such call (tests/test_piece_cases.py) -- and they are made in a child process, which also gives the
    two pinned and two device staging buffers of 256 MiB back when it ends."""
    results = in_a_child("cap", pc.cap_rows_set(), {})
    assert len(results) == 1 and results[0]["n"] == pc.CAP_N and results[0]["chunk"] == 4096
    assert not pc.failures(results), results


def test_vrf_verify_on_locked_and_pageable_arrays(lib):
    """ed25519_VRF_Verify_batch, the one list of five arrays, with pk, proof and beta page-locked (the copy engines work on the
    caller's memory: an int column and 80-byte rows the direct path has not seen) and alpha and ok pageable: the same bytes"""
    import torch
    arrays = pc.family_rows("vrf")
    n = pc.DEFAULT_N
    idx = np.arange(n) % len(arrays["pk_v"])
    pin = {k: torch.from_numpy(arrays[k][idx]).pin_memory() for k in ("pk_v", "pi_v")}
    beta = torch.full((n + 1, 64), pc.FILL, dtype=torch.uint8).pin_memory()
    alpha = np.ascontiguousarray(arrays["alpha_v"][idx])
    ok = np.full(n + 1, pc.FILL, np.uint8).repeat(4).view(np.int32)
    D = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.ed25519_VRF_Verify_batch(D(beta), C.c_void_p(ok.ctypes.data), D(pin["pk_v"]), D(pin["pi_v"]), C.c_void_p(alpha.ctypes.data),
                                        alpha.shape[1], n) == 0, lib.c25519_amd_last_error()
    got = beta.numpy()
    bad = np.flatnonzero((got[:n] != arrays["beta_v"][idx]).any(axis=1) | (ok[:n] != arrays["ok_v"][idx]))
    assert not len(bad), [(int(i), int(i) // 65536) for i in bad[:4]]
    assert (got[n] == pc.FILL).all() and ok[n:].view(np.uint8).tolist() == [pc.FILL] * 4, "the guard rows"
    assert np.array_equal(pin["pk_v"].numpy(), arrays["pk_v"][idx]) and np.array_equal(pin["pi_v"].numpy(), arrays["pi_v"][idx])
    assert np.array_equal(alpha, arrays["alpha_v"][idx])
