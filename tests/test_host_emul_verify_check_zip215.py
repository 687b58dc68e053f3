"""CPU tests of the coset comparison behind ed25519_Verify_Check_zip215_* (curve25519_amd/csrc/verify_ctx_zip215.cuh).  The device
source -- the coset prep's lane, the shared inversion's lanes with FinishVerifyZip215, the per-context rule 2 -- is compiled by g++
against the C model of the gfx950 primitives (tests/host_emul/verify_check_zip215.cpp, tests/host_emul/build.py's build_lib) and
judged element by element against tests/check_zip215_model.py, which supplies T = [S]B - [k]A in big integers, scaled by a Z != 1
of its choice.  Sets: ZIP-215's conformance grid, the torsion and degenerate sets, the generated torsion-shift set."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from host_emul.build import CSRC, assert_no_mad_overflow, open_lib
import check_zip215_model as cm
import zip215_cases as zc
from vectors import P, small_order_encodings

vp, sz = C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def lib():
    lib = open_lib({"emul_zip215_ctx_key_ok": ([vp], C.c_uint),
                    "emul_check_zip215_finish": ([vp, vp, vp, sz, vp, vp, sz, C.c_int], C.c_int)},
                   "verify_check_zip215.cpp", "libc25519_emul_verify_check_zip215.so")
    yield lib
    assert_no_mad_overflow(lib)


def points_for(sig, pk, msg, seed):
    """(xyz uint8[n, 96], key flags): the model's T scaled by a random Z != 1; a key that does not decode gets a point that is not
    on the curve and flag 0, as a Verify_Init context of it would give"""
    rnd = random.Random(seed)
    xyz, ok = np.zeros((len(sig), 96), np.uint8), np.zeros(len(sig), np.uint32)
    for i in range(len(sig)):
        T = cm.walk_point(sig[i], pk[i], msg[i])
        z = rnd.randrange(2, P)
        if T is None:
            T = (rnd.randrange(P), rnd.randrange(P))
        else:
            ok[i] = 1
        row = b"".join(v.to_bytes(32, "little") for v in (T[0] * z % P, T[1] * z % P, z))
        xyz[i] = np.frombuffer(row, np.uint8)
    return xyz, ok


def run(lib, xyz, sig, key_ok, idx=None, n_ctx=1, k=4):
    n = len(sig)
    out = np.full(n, -1, np.int32)
    xyz, sig, key_ok = (np.ascontiguousarray(a) for a in (xyz, sig, key_ok))
    idx = None if idx is None else np.ascontiguousarray(idx, np.uint32)
    lib.emul_check_zip215_finish(out.ctypes.data, xyz.ctypes.data, None if idx is None else idx.ctypes.data, n_ctx, key_ok.ctypes.data,
                                 sig.ctypes.data, n, k)
    return out


def judged(lib, sig, pk, msg, seed, k=4):
    """one context per element (index i, flag key_ok[i]) through the finish, against the model"""
    xyz, ok = points_for(sig, pk, msg, seed)
    got = run(lib, xyz, sig, ok, idx=np.arange(len(sig)), n_ctx=len(sig), k=k)
    return got, cm.model_verdicts(sig, pk, msg)


def test_header_constants_are_the_models():
    text = open(os.path.join(CSRC, "verify_ctx_zip215.cuh")).read()
    for name, val in (("K_T8X", cm.X8), ("K_T8Y", cm.Y8), ("K_T8K", cm.K8)):
        body = re.search(name + r"\[8\] = \{([^}]*)\}", text).group(1)
        assert [int(w.strip().rstrip("u"), 16) for w in body.split(",")] == cm.words(val), name


def test_conformance_grid(lib):
    sig, pk, msg = zc.conformance_grid()
    got, exp = judged(lib, sig, pk, msg, 1)
    assert exp.all() and np.array_equal(got, exp)


def test_torsion_degenerate_and_generated_sets(lib):
    for seed, (sig, pk, msg) in enumerate((zc.torsion(), zc.degenerate()[:3], cm.generated_set()[:3])):
        got, exp = judged(lib, sig, pk, msg, 10 + seed)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (seed, bad[:10], got[bad[:10]], exp[bad[:10]])
        assert exp.any()


def test_every_group_size_and_a_tail(lib):
    """the shared inversion at every group size this finish is instantiated for, with n no multiple of 4 K"""
    sig, pk, msg, _ = cm.generated_set()
    sig, pk, msg = sig[:131], pk[:131], msg[:131]
    xyz, ok = points_for(sig, pk, msg, 20)
    exp = cm.model_verdicts(sig, pk, msg)
    for k in (1, 2, 4, 8, 12):
        assert np.array_equal(run(lib, xyz, sig, ok, idx=np.arange(131), n_ctx=131, k=k), exp), k


def test_zero_point_and_bad_index_give_zero(lib):
    """Z = 0 -- the zero point an index out of range leaves, or any (X, Y, 0) -- gives 0 also where R = 32 zero bytes (the candidates
    would all be (0, 0), and x = 0 ignores the sign bit); so does an index out of range over a valid element, and a cleared key flag"""
    sig, pk, msg = zc.conformance_grid()
    sig, pk, msg = sig[:16].copy(), pk[:16], msg[:16]
    xyz, ok = points_for(sig, pk, msg, 30)
    assert run(lib, xyz, sig, ok, idx=np.arange(16), n_ctx=16).all()
    zero = xyz.copy()
    zero[:8] = 0
    zero[8:, 64:] = 0
    zsig = sig.copy()
    zsig[:, :32] = 0
    zsig[1::2, 31] = 0x80
    assert not run(lib, zero, zsig, ok, idx=np.arange(16), n_ctx=16).any()
    idx = np.arange(16, dtype=np.uint32)
    idx[[3, 7]] = (16, 0xFFFFFFFF)
    got = run(lib, xyz, sig, ok, idx=idx, n_ctx=16)
    assert not got[[3, 7]].any() and np.delete(got, [3, 7]).all()
    ok2 = ok.copy()
    ok2[5] = 0
    got = run(lib, xyz, sig, ok2, idx=np.arange(16), n_ctx=16)
    assert got[5] == 0 and np.delete(got, 5).all()
    one = run(lib, xyz, sig, np.ones(1, np.uint32), idx=None, n_ctx=1)      # one context: flag 0 for everyone
    assert one.all()


def test_rule_2_from_the_context(lib, oracle):
    """zip215_ctx_key_ok on orc_ed25519_verify_init's contexts (Verify_Init's layout and decoding): 1 exactly where the key decodes
    -- honest keys, every small-order encoding (x = 0 with the sign bit, y + p), y >= p -- and 0 where it does not"""
    L = oracle.lib
    L.orc_ed25519_verify_init.argtypes = [vp, vp]
    L.orc_ed25519_verify_init.restype = None
    rng = np.random.default_rng(0x2152)
    pub, _ = oracle.ed25519_keypair(rng.integers(0, 256, (4, 32), dtype=np.uint8))
    keys = [bytes(p) for p in pub] + [e for e, _ in small_order_encodings()] + cm.undecodable_strings(6, 7)
    keys += [bytes(r) for r in zc.noncanonical_y_strings()]
    seen = set()
    for kb in keys:
        pkb = np.frombuffer(kb, np.uint8).copy()
        ctx = np.zeros(2080, np.uint8)
        L.orc_ed25519_verify_init(ctx.ctypes.data, pkb.ctypes.data)
        exp = int(zc.zip215_decode(kb) is not None)
        assert lib.emul_zip215_ctx_key_ok(ctx.ctypes.data) == exp, kb.hex()
        seen.add(exp)
        if exp:                                                 # a context that is not Verify_Init's any more: a flipped bit in row 1's x
            ctx[32 + 128 + 3] ^= 4
            assert lib.emul_zip215_ctx_key_ok(ctx.ctypes.data) == 0
    assert seen == {0, 1}
