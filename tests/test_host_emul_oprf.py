"""CPU tests of the OPRF / VOPRF calls' lane functions (curve25519_amd/csrc/oprf25519.cuh: what ristretto255_OPRF_Blind_*,
ristretto255_OPRF_Finalize_*, ristretto255_OPRF_BlindEvaluate_*, ristretto255_VOPRF_BlindEvaluate_* and ristretto255_VOPRF_VerifyProof_*
run on the device, and the host's oprf_make_tail in front of them).  The device source is compiled by g++ against the C model of the
gfx950 primitives (tests/host_emul/oprf.cpp, tests/host_emul/build.py's open_lib) and judged byte for byte against the big-integer
model of RFC 9497 (tests/oprf_model.py) on the case set the GPU tests share (tests/oprf_checks.py) and on the published vectors."""
import ctypes as C

import numpy as np
import pytest

from host_emul.build import assert_no_mad_overflow, open_lib
import oprf_checks as checks
import oprf_model as model

vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int


def _c(a):
    return np.ascontiguousarray(a)


def _key(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


class Emulated:
    def __init__(self, lib):
        self.lib = lib

    def blind(self, inp, blind, mode):
        n = len(blind)
        inp, blind = _c(inp), _c(blind)
        before = (inp.copy(), blind.copy())
        out, ok = np.full((n, 32), 0xA5, np.uint8), np.full(n, -1, np.int32)
        self.lib.emul_oprf_blind(out.ctypes.data, ok.ctypes.data, inp.ctypes.data, inp.shape[1], blind.ctypes.data, mode, n)
        assert np.array_equal(inp, before[0]) and np.array_equal(blind, before[1])
        return out, ok

    def finalize(self, inp, blind, evaluated):
        n = len(blind)
        inp, blind, evaluated = _c(inp), _c(blind), _c(evaluated)
        before = (inp.copy(), blind.copy(), evaluated.copy())
        out, ok = np.full((n, 64), 0xA5, np.uint8), np.full(n, -1, np.int32)
        self.lib.emul_oprf_finalize(out.ctypes.data, ok.ctypes.data, inp.ctypes.data, inp.shape[1], blind.ctypes.data, evaluated.ctypes.data, n)
        assert all(np.array_equal(a, b) for a, b in zip((inp, blind, evaluated), before))
        return out, ok

    def evaluate(self, sks, blinded):
        n = len(blinded)
        k, blinded = _key(sks), _c(blinded)
        before = (k.copy(), blinded.copy())
        out, ok = np.full((n, 32), 0xA5, np.uint8), np.full(n, -1, np.int32)
        self.lib.emul_oprf_evaluate(out.ctypes.data, ok.ctypes.data, k.ctypes.data, blinded.ctypes.data, n)
        assert np.array_equal(k, before[0]) and np.array_equal(blinded, before[1])
        return out, ok

    def voprf_evaluate(self, sks, proof_rand, blinded, offsets):
        m, n = len(proof_rand), len(blinded)
        k, proof_rand, blinded, offsets = _key(sks), _c(proof_rand), _c(blinded), _c(np.asarray(offsets, np.uint64))
        before = (k.copy(), proof_rand.copy(), blinded.copy(), offsets.copy())
        evaluated, proof = np.full((n, 32), 0xA5, np.uint8), np.full((m, 64), 0xA5, np.uint8)
        ok, req_ok = np.full(n, -1, np.int32), np.full(m, -1, np.int32)
        self.lib.emul_voprf_evaluate(evaluated.ctypes.data, proof.ctypes.data, ok.ctypes.data, req_ok.ctypes.data, k.ctypes.data,
                                     proof_rand.ctypes.data, blinded.ctypes.data, offsets.ctypes.data, m, n)
        assert all(np.array_equal(a, b) for a, b in zip((k, proof_rand, blinded, offsets), before))
        return evaluated, proof, ok, req_ok

    def voprf_verify(self, pks, blinded, evaluated, proof, offsets):
        m, n = len(proof), len(blinded)
        k, blinded, evaluated, proof = _key(pks), _c(blinded), _c(evaluated), _c(proof)
        offsets = _c(np.asarray(offsets, np.uint64))
        before = (k.copy(), blinded.copy(), evaluated.copy(), proof.copy(), offsets.copy())
        req_ok = np.full(m, -1, np.int32)
        self.lib.emul_voprf_verify(req_ok.ctypes.data, k.ctypes.data, blinded.ctypes.data, evaluated.ctypes.data, proof.ctypes.data,
                                   offsets.ctypes.data, m, n)
        assert all(np.array_equal(a, b) for a, b in zip((k, blinded, evaluated, proof, offsets), before))
        return req_ok


@pytest.fixture(scope="module")
def impl():
    lib = open_lib({"emul_oprf_blind": ([vp, vp, vp, sz, vp, ci, sz], None), "emul_oprf_finalize": ([vp, vp, vp, sz, vp, vp, sz], None),
                    "emul_oprf_evaluate": ([vp, vp, vp, vp, sz], None),
                    "emul_voprf_evaluate": ([vp, vp, vp, vp, vp, vp, vp, vp, sz, sz], None),
                    "emul_voprf_verify": ([vp, vp, vp, vp, vp, vp, sz, sz], None)}, "oprf.cpp", "libc25519_emul_oprf.so")
    yield Emulated(lib)
    assert_no_mad_overflow(lib)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("length", model.INPUT_LENGTHS)
def test_honest_rows_match_the_model(impl, length, mode):
    checks.honest_rows(impl, length, mode)


def test_rejected_rows_match_the_model(impl):
    checks.row_rejections(impl)


def test_the_published_vectors_end_to_end(impl):
    checks.vectors_end_to_end(impl)


@pytest.mark.parametrize("shuffled", (False, True))
def test_every_request_size_in_one_call(impl, shuffled):
    checks.request_sizes(impl, shuffled)


def test_the_server_rejects_what_the_model_rejects(impl):
    checks.server_rejections(impl)


def test_the_verifier_rejects_what_the_model_rejects(impl):
    checks.verify_rejections(impl)


def test_malformed_offsets_fail_their_requests_only(impl):
    checks.malformed_offsets(impl)
