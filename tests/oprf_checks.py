"""The checks the CPU emulation and the GPU tests of the OPRF / VOPRF calls share: each takes an implementation -- an object with
blind, finalize, evaluate, voprf_evaluate and voprf_verify over numpy arrays, which fills its outputs with 0xA5 / -1 before the call
and asserts its inputs unchanged after it -- and holds it byte for byte against tests/oprf_model.py on the case set and the
published vectors."""
import numpy as np

import oprf_model as model
from oprf_model import _rows


def _bad(labels, got, want):
    return [(lab, int(g), int(w)) for lab, g, w in zip(labels, got, want) if int(g) != int(w)]


def honest_rows(impl, length, mode):
    h = model.honest(length, mode)
    blinded, ok = impl.blind(h["input"], h["blind"], mode)
    assert ok.tolist() == [1] * len(ok) and np.array_equal(blinded, h["blinded"]), (length, mode)
    evaluated, ok = impl.evaluate(model.SKS, h["blinded"])
    assert ok.tolist() == [1] * len(ok) and np.array_equal(evaluated, h["evaluated"]), (length, mode)
    output, ok = impl.finalize(h["input"], h["blind"], h["evaluated"])
    assert ok.tolist() == [1] * len(ok) and np.array_equal(output, h["output"]), (length, mode)


def row_rejections(impl):
    rows = model.row_rejections()
    labels = [r[2] for r in rows]
    points, blinds = _rows([r[0] for r in rows], 32), _rows([r[1] for r in rows], 32)
    # the server's row rule: the point column under the case set's key, and under a key of 0 and of L
    for sks in (model.SKS, model.ZERO32, model._le(model.L)):
        want = [model.evaluate_row(sks, r[0]) for r in rows]
        evaluated, ok = impl.evaluate(sks, points)
        assert not _bad(labels, ok, [w[1] for w in want]), (sks.hex(), _bad(labels, ok, [w[1] for w in want]))
        assert np.array_equal(evaluated, _rows([w[0] for w in want], 32)), sks.hex()
    # Finalize: the point column as `evaluated`, the blind column as the blind
    inputs = _rows([model._seeded(5, "reject input %d" % k) for k in range(len(rows))], 5)
    want = [model.finalize(bytes(i), r[1], r[0]) for i, r in zip(inputs, rows)]
    assert {w[2] for w in want} == {"valid", "evaluated does not decode", "evaluated is the identity", "blind is zero"}
    output, ok = impl.finalize(inputs, blinds, points)
    assert not _bad(labels, ok, [w[1] for w in want]), _bad(labels, ok, [w[1] for w in want])
    assert np.array_equal(output, _rows([w[0] for w in want], 64))
    # Blind: the blind column
    for mode in (0, 1):
        want = [model.blind(bytes(i), r[1], mode) for i, r in zip(inputs, rows)]
        assert [w[1] for w in want].count(0) == 2
        blinded, ok = impl.blind(inputs, blinds, mode)
        assert not _bad(labels, ok, [w[1] for w in want]), (mode, _bad(labels, ok, [w[1] for w in want]))
        assert np.array_equal(blinded, _rows([w[0] for w in want], 32)), mode


def vectors_end_to_end(impl):
    """Blind, VOPRF_BlindEvaluate, VerifyProof, Finalize on the three mode-1 vectors, and the mode-0 vector through Blind, BlindEvaluate,
    Finalize"""
    sks, pks = bytes.fromhex(model.VOPRF_SKS), bytes.fromhex(model.VOPRF_PKS)
    for v in model.VECTORS:
        n = len(v["inputs"])
        blinds = _rows([bytes.fromhex(b) for b in v["blinds"]], 32)
        blinded = []
        for inp, b in zip(v["inputs"], blinds):                      # (one length per call)
            out, ok = impl.blind(_rows([inp], len(inp)), b.reshape(1, 32), 1)
            assert ok.tolist() == [1]
            blinded.append(out[0])
        blinded = np.stack(blinded)
        assert [r.tobytes().hex() for r in blinded] == list(v["blinded"])
        off = np.array([0, n], np.uint64)
        evaluated, proof, ok, req_ok = impl.voprf_evaluate(sks, _rows([bytes.fromhex(v["r"])], 32), blinded, off)
        assert ok.tolist() == [1] * n and req_ok.tolist() == [1]
        assert [r.tobytes().hex() for r in evaluated] == list(v["evaluated"])
        assert proof.tobytes().hex() == v["proof"]
        assert impl.voprf_verify(pks, blinded, evaluated, proof, off).tolist() == [1]
        for inp, b, e, want in zip(v["inputs"], blinds, evaluated, v["outputs"]):
            out, ok = impl.finalize(_rows([inp], len(inp)), b.reshape(1, 32), e.reshape(1, 32))
            assert ok.tolist() == [1] and out.tobytes().hex() == want
    import test_h2c_model as a11
    inp = _rows([a11.OPRF_INPUT], 1)
    b = _rows([bytes.fromhex(a11.OPRF_BLIND)], 32)
    blinded, ok = impl.blind(inp, b, 0)
    assert ok.tolist() == [1] and blinded.tobytes().hex() == a11.OPRF_BLINDED
    evaluated, ok = impl.evaluate(bytes.fromhex(a11.OPRF_SKS), blinded)
    assert ok.tolist() == [1] and evaluated.tobytes().hex() == a11.OPRF_EVALUATION
    out, ok = impl.finalize(inp, b, evaluated)
    assert ok.tolist() == [1] and out.tobytes().hex() == a11.OPRF_OUTPUT


def request_sizes(impl, shuffled):
    c = model.request_case(shuffled)
    m, n = len(c["sizes"]), len(c["blinded"])
    evaluated, proof, ok, req_ok = impl.voprf_evaluate(model.SKS, c["proof_rand"], c["blinded"], c["offsets"])
    assert ok.tolist() == [1] * n and req_ok.tolist() == [1] * m, (c["sizes"], req_ok.tolist())
    assert np.array_equal(evaluated, c["evaluated"])
    bad = [s for s, g, w in zip(c["sizes"], proof, c["proof"]) if not np.array_equal(g, w)]
    assert not bad, bad
    assert impl.voprf_verify(c["pks"], c["blinded"], c["evaluated"], c["proof"], c["offsets"]).tolist() == [1] * m


def server_rejections(impl):
    for case in model.server_rejections():
        w = case["want"]
        evaluated, proof, ok, req_ok = impl.voprf_evaluate(case["sks"], case["proof_rand"], case["blinded"], case["offsets"])
        assert ok.tolist() == w["ok"] and req_ok.tolist() == w["req_ok"], (case["label"], ok.tolist(), req_ok.tolist())
        assert np.array_equal(evaluated, w["evaluated"]) and np.array_equal(proof, w["proof"]), case["label"]


def verify_rejections(impl):
    for case in model.verify_rejections():
        got = impl.voprf_verify(case["pks"], case["blinded"], case["evaluated"], case["proof"], case["offsets"])
        assert got.tolist() == case["want"], (case["label"], got.tolist())


def malformed_offsets(impl):
    """the forms that take offsets as they come (the device's): the requests the label names fail, the others are the model's"""
    honest = model.server_rejections()[0]
    n, m = len(honest["blinded"]), len(honest["proof_rand"])
    blinded = [bytes(r) for r in honest["blinded"]]
    rand = [bytes(r) for r in honest["proof_rand"]]
    for label, off, must_fail in model.malformed_offsets() + (("a request of 65 536 rows", [0, 3, 5, 9, 9 + 65536], (3,)),):
        off = np.array(off, np.uint64)
        want = model.voprf_blind_evaluate(model.SKS, rand, blinded, off)
        assert all(want[3][j] == 0 for j in must_fail), label
        evaluated, proof, ok, req_ok = impl.voprf_evaluate(model.SKS, honest["proof_rand"], honest["blinded"], off)
        assert ok.tolist() == list(want[2]) and req_ok.tolist() == list(want[3]), (label, ok.tolist(), req_ok.tolist())
        assert np.array_equal(evaluated, _rows(want[0], 32)) and np.array_equal(proof, _rows(want[1], 64)), label
        # the verifier on what the model's server made of these offsets, and on the honest call's outputs under them
        for ev, pr in ((want[0], want[1]), (honest["want"]["evaluated"], honest["want"]["proof"])):
            wv = model.voprf_verify(model.base_mult(model.KEY), blinded, [bytes(r) for r in ev], [bytes(r) for r in pr], off)
            assert all(wv[j] == 0 for j in must_fail), label
            got = impl.voprf_verify(model.base_mult(model.KEY), honest["blinded"], _rows(ev, 32), _rows(pr, 64), off)
            assert got.tolist() == wv, (label, got.tolist(), wv)
    assert n == sum(model.REJECT_SIZES) and m == len(model.REJECT_SIZES)
