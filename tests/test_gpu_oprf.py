"""GPU suite (MI355X): ristretto255_OPRF_Blind_*, ristretto255_OPRF_Finalize_*, ristretto255_OPRF_BlindEvaluate_*,
ristretto255_VOPRF_BlindEvaluate_* and ristretto255_VOPRF_VerifyProof_* (RFC 9497, ristretto255-SHA512, modes 0x00 and 0x01).  Every
output must be the bytes of the big-integer model (tests/oprf_model.py, pinned to the published vectors by tests/test_oprf_model.py) on
the case set the CPU tests share (tests/oprf_checks.py), through the _dev forms and through the _batch forms of curve25519_amd.oprf;
the vectors must run end to end on the device; the calls must write every row and nothing behind the last one, leave their inputs
alone, work on another stream and replay from a captured graph; the three per-row calls must survive being cut into pipeline
pieces; and one proof over 65 535 rows must be the model's, while 65 536 rows are refused.  Byte-exact: no tolerance is involved."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oprf_checks as checks
import oprf_model as model
import piece_cases as pc
from curve25519_amd import _lib
from scalar_model import cycled

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, OK_FILL = 0xA5, 0x5A5A5A5A


@pytest.fixture(scope="module")
def oprf():
    import torch
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    from curve25519_amd import api, oprf as o
    assert api.device_count() >= 1
    return o


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a, dtype=np.uint8):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, copy=True)).to(dev())


def key_dev(b):
    return to_dev(np.frombuffer(bytes(b), np.uint8).reshape(1, 32))


def offsets_dev(offsets):
    return to_dev(np.asarray(offsets, np.uint64).astype(np.int64).reshape(-1, 1), np.int64)


def filled(n, width):
    import torch
    return torch.full((n + 1, width), FILL, dtype=torch.uint8, device=dev())


def ok_rows(n):
    import torch
    return torch.full((n + 1, 1), OK_FILL, dtype=torch.int32, device=dev())


def _back(outs, oks, ins):
    """the outputs of a device call without their guard rows, after the inputs were seen unchanged and the guards untouched"""
    import torch
    torch.cuda.synchronize()
    for t, a in ins:
        assert np.array_equal(t.cpu().numpy().reshape(np.asarray(a).shape), a), "inputs are never written"
    got = []
    for t in outs:
        a = t.cpu().numpy()
        assert (a[-1] == FILL).all(), "nothing is written behind the last row"
        got.append(a[:-1])
    for t in oks:
        a = t.cpu().numpy().reshape(-1)
        assert a[-1] == OK_FILL, "nothing is written behind the last row"
        got.append(a[:-1])
    return got


class OnDevice:
    """the _dev forms on torch tensors"""

    def __init__(self, oprf):
        self.o = oprf

    def blind(self, inp, blind, mode):
        n = len(blind)
        d_in, d_bl, d_out, d_ok = to_dev(inp), to_dev(blind), filled(n, 32), ok_rows(n)
        self.o.ristretto255_OPRF_Blind_dev(d_out[:n], d_ok[:n], d_in, d_bl, mode)
        return _back([d_out], [d_ok], [(d_in, inp), (d_bl, blind)])

    def finalize(self, inp, blind, evaluated):
        n = len(blind)
        d_in, d_bl, d_ev, d_out, d_ok = to_dev(inp), to_dev(blind), to_dev(evaluated), filled(n, 64), ok_rows(n)
        self.o.ristretto255_OPRF_Finalize_dev(d_out[:n], d_ok[:n], d_in, d_bl, d_ev)
        return _back([d_out], [d_ok], [(d_in, inp), (d_bl, blind), (d_ev, evaluated)])

    def evaluate(self, sks, blinded):
        n = len(blinded)
        d_k, d_bl, d_out, d_ok = key_dev(sks), to_dev(blinded), filled(n, 32), ok_rows(n)
        self.o.ristretto255_OPRF_BlindEvaluate_dev(d_out[:n], d_ok[:n], d_k, d_bl)
        return _back([d_out], [d_ok], [(d_k, np.frombuffer(bytes(sks), np.uint8).reshape(1, 32)), (d_bl, blinded)])

    def voprf_evaluate(self, sks, proof_rand, blinded, offsets):
        m, n = len(proof_rand), len(blinded)
        d_k, d_r, d_bl, d_off = key_dev(sks), to_dev(proof_rand), to_dev(blinded), offsets_dev(offsets)
        d_ev, d_pr, d_ok, d_rok = filled(n, 32), filled(m, 64), ok_rows(n), ok_rows(m)
        self.o.ristretto255_VOPRF_BlindEvaluate_dev(d_ev[:n], d_pr[:m], d_ok[:n], d_rok[:m], d_k, d_r, d_bl, d_off)
        key = np.frombuffer(bytes(sks), np.uint8).reshape(1, 32)
        ev, pr, ok, rok = _back([d_ev, d_pr], [d_ok, d_rok], [(d_k, key), (d_r, proof_rand), (d_bl, blinded)])
        assert np.array_equal(d_off.cpu().numpy().reshape(-1).astype(np.uint64), np.asarray(offsets, np.uint64))
        return ev, pr, ok, rok

    def voprf_verify(self, pks, blinded, evaluated, proof, offsets):
        m, n = len(proof), len(blinded)
        d_k, d_bl, d_ev, d_pr, d_off, d_rok = key_dev(pks), to_dev(blinded), to_dev(evaluated), to_dev(proof), offsets_dev(offsets), ok_rows(m)
        self.o.ristretto255_VOPRF_VerifyProof_dev(d_rok[:m], d_k, d_bl, d_ev, d_pr, d_off)
        ins = [(d_k, np.frombuffer(bytes(pks), np.uint8).reshape(1, 32)), (d_bl, blinded), (d_ev, evaluated), (d_pr, proof)]
        rok = _back([], [d_rok], ins)[0]
        assert np.array_equal(d_off.cpu().numpy().reshape(-1).astype(np.uint64), np.asarray(offsets, np.uint64))
        return rok


class OnHost:
    """the _batch forms through curve25519_amd.oprf's numpy wrappers"""

    def __init__(self, oprf):
        self.o = oprf

    @staticmethod
    def _unchanged(call, *ins):
        before = [np.array(a, copy=True) for a in ins]
        out = call()
        assert all(np.array_equal(a, b) for a, b in zip(ins, before)), "inputs are never written"
        return out

    def blind(self, inp, blind, mode):
        return self._unchanged(lambda: self.o.ristretto255_OPRF_Blind(inp, blind, mode), inp, blind)

    def finalize(self, inp, blind, evaluated):
        return self._unchanged(lambda: self.o.ristretto255_OPRF_Finalize(inp, blind, evaluated), inp, blind, evaluated)

    def evaluate(self, sks, blinded):
        return self._unchanged(lambda: self.o.ristretto255_OPRF_BlindEvaluate(np.frombuffer(bytes(sks), np.uint8), blinded), blinded)

    def voprf_evaluate(self, sks, proof_rand, blinded, offsets):
        return self._unchanged(lambda: self.o.ristretto255_VOPRF_BlindEvaluate(np.frombuffer(bytes(sks), np.uint8), proof_rand, blinded, offsets),
                               proof_rand, blinded, offsets)

    def voprf_verify(self, pks, blinded, evaluated, proof, offsets):
        return self._unchanged(lambda: self.o.ristretto255_VOPRF_VerifyProof(np.frombuffer(bytes(pks), np.uint8), blinded, evaluated, proof, offsets),
                               blinded, evaluated, proof, offsets)


@pytest.fixture(scope="module", params=("dev", "batch"))
def impl(request, oprf):
    return OnDevice(oprf) if request.param == "dev" else OnHost(oprf)


@pytest.mark.parametrize("mode", (0, 1))
def test_honest_rows_at_every_input_length(impl, mode):
    for length in model.INPUT_LENGTHS:
        checks.honest_rows(impl, length, mode)


def test_rejected_rows(impl):
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


def test_malformed_offsets_fail_their_requests_on_the_device(oprf):
    checks.malformed_offsets(OnDevice(oprf))


def test_malformed_offsets_are_bad_arguments_to_the_host_forms(oprf):
    lib = _lib.load()
    honest = model.server_rejections()[0]
    n, m = len(honest["blinded"]), len(honest["proof_rand"])
    sks = np.frombuffer(model.SKS, np.uint8).copy()
    pks = np.frombuffer(model.base_mult(model.KEY), np.uint8).copy()
    ev, pr = np.full((n, 32), FILL, np.uint8), np.full((m, 64), FILL, np.uint8)
    ok, rok = np.full(n, OK_FILL, np.int32), np.full(m, OK_FILL, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    cases = model.malformed_offsets() + (("a request of 65 536 rows", [0, 3, 5, 9, 9 + 65536], (3,)),)
    for label, off, _ in cases:
        off = np.array(off, np.uint64)
        rc = lib.ristretto255_VOPRF_BlindEvaluate_batch(p(ev), p(pr), p(ok), p(rok), p(sks), p(honest["proof_rand"]), p(honest["blinded"]), p(off), m, n)
        assert rc != 0 and lib.c25519_amd_last_error() != b"", label
        rc = lib.ristretto255_VOPRF_VerifyProof_batch(p(rok), p(pks), p(honest["blinded"]), p(honest["want"]["evaluated"]),
                                                      p(honest["want"]["proof"]), p(off), m, n)
        assert rc != 0 and lib.c25519_amd_last_error() != b"", label
        with pytest.raises(ValueError):
            oprf.ristretto255_VOPRF_BlindEvaluate(sks, honest["proof_rand"], honest["blinded"], off)
    assert (ev == FILL).all() and (pr == FILL).all() and (ok == OK_FILL).all() and (rok == OK_FILL).all(), "a refused call writes nothing"


def test_another_stream_and_a_captured_graph(oprf):
    """the whole protocol for 300 rows in five requests on a side stream, then captured and replayed: the proof calls are three
    kernels over leased scratch and allocate nothing once the slab exists"""
    import torch
    n, sizes = 300, (1, 64, 100, 35, 100)
    h = model.honest(67, 1)
    inp, bl = cycled(h["input"], n), cycled(h["blind"], n)
    off = model.request_offsets(sizes)
    m = len(sizes)
    rand = model._rows([model._le(model._scalar("stream rand %d" % j)) for j in range(m)], 32)
    blinded = cycled(h["blinded"], n)
    want = model.voprf_blind_evaluate(model.SKS, [bytes(r) for r in rand], [bytes(r) for r in blinded], off)
    assert want[3] == [1] * m
    output = cycled(h["output"], n)
    d_in, d_bl, d_k, d_pk, d_r, d_off = to_dev(inp), to_dev(bl), key_dev(model.SKS), key_dev(model.base_mult(model.KEY)), to_dev(rand), offsets_dev(off)
    d_blinded, d_ev, d_pr, d_out = filled(n, 32), filled(n, 32), filled(m, 64), filled(n, 64)
    d_ok = [ok_rows(n) for _ in range(3)]
    d_rok = [ok_rows(m) for _ in range(2)]
    side = torch.cuda.Stream(dev())

    def step():
        oprf.ristretto255_OPRF_Blind_dev(d_blinded[:n], d_ok[0][:n], d_in, d_bl, 1)
        oprf.ristretto255_VOPRF_BlindEvaluate_dev(d_ev[:n], d_pr[:m], d_ok[1][:n], d_rok[0][:m], d_k, d_r, d_blinded[:n], d_off)
        oprf.ristretto255_VOPRF_VerifyProof_dev(d_rok[1][:m], d_pk, d_blinded[:n], d_ev[:n], d_pr[:m], d_off)
        oprf.ristretto255_OPRF_Finalize_dev(d_out[:n], d_ok[2][:n], d_in, d_bl, d_ev[:n])

    def check():
        torch.cuda.synchronize()
        assert np.array_equal(d_blinded.cpu().numpy()[:n], blinded) and (d_blinded.cpu().numpy()[n] == FILL).all()
        assert np.array_equal(d_ev.cpu().numpy()[:n], model._rows(want[0], 32))
        assert np.array_equal(d_pr.cpu().numpy()[:m], model._rows(want[1], 64)) and (d_pr.cpu().numpy()[m] == FILL).all()
        assert np.array_equal(d_out.cpu().numpy()[:n], output)
        assert all((t.cpu().numpy()[:-1] == 1).all() and t.cpu().numpy()[-1] == OK_FILL for t in d_ok + d_rok)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        step()
    side.synchronize()
    check()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    for t in (d_blinded, d_ev, d_pr, d_out):
        t.fill_(FILL)
    for t in d_ok + d_rok:
        t.fill_(OK_FILL)
    torch.cuda.synchronize()
    g.replay()
    check()


# the child of the pieces test: the period rows arrive in a small .npz, are cycled to n rows there, every call runs through the C
# ABI into n + 1 rows of FILL, and one JSON line of what went wrong comes back
CHILD = (
    "import ctypes as C, json, sys; sys.path[:0] = [%r, %r]\n"
    "import numpy as np\n"
    "from curve25519_amd import _lib\n"
    "from scalar_model import cycled\n"
    "a = dict(np.load(sys.argv[1])); n = int(sys.argv[2]); lib = _lib.load(); bad = []\n"
    "p = lambda x: C.c_void_p(x.ctypes.data)\n"
    "inp, bl, blinded, ev, out = (cycled(a[k], n) for k in ('input', 'blind', 'blinded', 'evaluated', 'output'))\n"
    "def run(name, call, width, want):\n"
    "    got, ok = np.full((n + 1, width), 0xA5, np.uint8), np.full(n + 1, 0x5A5A5A5A, np.int32)\n"
    "    rc = call(got, ok)\n"
    "    if rc or not np.array_equal(got[:n], want) or not (ok[:n] == 1).all() or not (got[n] == 0xA5).all() or ok[n] != 0x5A5A5A5A:\n"
    "        rows = np.nonzero((got[:n] != want).any(axis=1))[0]\n"
    "        bad.append([name, int(rc), int(len(rows)), int(rows[0]) if len(rows) else -1])\n"
    "run('blind', lambda g, ok: lib.ristretto255_OPRF_Blind_batch(p(g), p(ok), p(inp), inp.shape[1], p(bl), 1, n), 32, blinded)\n"
    "run('evaluate', lambda g, ok: lib.ristretto255_OPRF_BlindEvaluate_batch(p(g), p(ok), p(a['sks']), p(blinded), n), 32, ev)\n"
    "run('finalize', lambda g, ok: lib.ristretto255_OPRF_Finalize_batch(p(g), p(ok), p(inp), inp.shape[1], p(bl), p(ev), n), 64, out)\n"
    "print(json.dumps(bad))\n") % (ROOT, os.path.join(ROOT, "tests"))
PIECE_PERIOD = 53                                   # prime, and no divisor of a piece's 5632 rows: a misplaced piece shows
PIECE_INPUT = 67


def test_the_per_row_calls_cut_into_pieces(oprf):
    """CUT_N rows in a fresh process under piece_cases.CUT_KNOBS (the knobs are read once per process): 24 pieces over 8 buffer sets,
    three stagers and two drainers, the server's key uploaded once for all of them"""
    assert pc.PIECE_SIZES[0] % PIECE_PERIOD and pc.CUT_N > pc.PIECE_THRESHOLD
    inp = [model._seeded(PIECE_INPUT, "piece input %d" % k) for k in range(PIECE_PERIOD)]
    bl = [model._le(model._scalar("piece blind %d" % k)) for k in range(PIECE_PERIOD)]
    blinded = [model.blind(i, b, 1)[0] for i, b in zip(inp, bl)]
    ev = [model.evaluate_row(model.SKS, b)[0] for b in blinded]
    out = [model.finalize(i, b, e)[0] for i, b, e in zip(inp, bl, ev)]
    arrays = dict(input=model._rows(inp, PIECE_INPUT), blind=model._rows(bl, 32), blinded=model._rows(blinded, 32), evaluated=model._rows(ev, 32),
                  output=model._rows(out, 64), sks=np.frombuffer(model.SKS, np.uint8))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rows.npz")
        np.savez(path, **arrays)
        p = subprocess.run([sys.executable, "-c", CHILD, path, str(pc.CUT_N)], capture_output=True, text=True, timeout=240,
                           env={**os.environ, **pc.CUT_KNOBS})
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == []


def test_one_proof_over_65535_rows_and_none_over_65536(oprf):
    """C_i = [a_i]B from ristretto255_ScalarMultBase_dev for 65 536 seeded a_i; the server's proof over the first 65 535 is the model's
    with d_i hashed here and M = [sum a_i d_i]B, Z = [skS]M from one multiplication each; VerifyProof accepts it; the same calls with
    all 65 536 rows in the request give req_ok = 0"""
    import torch
    from curve25519_amd import api
    big, n = model.MAX_ROWS, model.MAX_ROWS + 1
    rng = np.random.default_rng(0x65535)
    a_rows = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    a_rows[:, 31] &= 0x0f                            # below 2^252 < L: the scalar is its own residue
    logs = [int.from_bytes(r.tobytes(), "little") for r in a_rows]
    d_a, d_c = to_dev(a_rows), filled(n, 32)
    api.ristretto255_ScalarMultBase_dev(d_c[:n], d_a)
    d_k, d_pk = key_dev(model.SKS), key_dev(model.base_mult(model.KEY))
    rand = model._rows([model._le(model._scalar("big rand"))], 32)
    d_r = to_dev(rand)
    for rows, want_ok in ((big, 1), (n, 0)):
        d_off = offsets_dev([0, rows])
        d_ev, d_pr, d_ok, d_rok, d_vok = filled(rows, 32), filled(1, 64), ok_rows(rows), ok_rows(1), ok_rows(1)
        oprf.ristretto255_VOPRF_BlindEvaluate_dev(d_ev[:rows], d_pr[:1], d_ok[:rows], d_rok[:1], d_k, d_r, d_c[:rows], d_off)
        oprf.ristretto255_VOPRF_VerifyProof_dev(d_vok[:1], d_pk, d_c[:rows], d_ev[:rows], d_pr[:1], d_off)
        torch.cuda.synchronize()
        assert d_rok.cpu().numpy().reshape(-1).tolist() == [want_ok, OK_FILL] and d_vok.cpu().numpy().reshape(-1).tolist() == [want_ok, OK_FILL]
        proof = d_pr.cpu().numpy()
        assert (proof[1] == FILL).all()
        if not want_ok:
            assert not proof[0].any() and not d_ok.cpu().numpy()[:rows].any() and not d_ev.cpu().numpy()[:rows].any()
            continue
        assert (d_ok.cpu().numpy()[:rows] == 1).all()
        cs, ds = d_c.cpu().numpy()[:rows], d_ev.cpu().numpy()[:rows]
        assert ds[0].tobytes() == model.evaluate_row(model.SKS, cs[0].tobytes())[0]
        assert ds[-1].tobytes() == model.evaluate_row(model.SKS, cs[-1].tobytes())[0]
        want = model.generate_proof(model.KEY, model.base_mult(model.KEY), [r.tobytes() for r in cs], [r.tobytes() for r in ds],
                                    model._int(rand[0].tobytes()), logs[:rows])
        assert proof[0].tobytes() == want
