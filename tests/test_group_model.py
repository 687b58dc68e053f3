"""The big-integer model of the group calls (tests/group_model.py) checked against itself and pinned to the compiled reference --
not to the code under test: for clamped scalars the Montgomery u of the model's [e]P is the oracle's X25519 shared secret of u(P),
and ScalarMultBase of a seed's scalar is the golden file's Ed25519 public key.  Also the recoding's digit counts, which the device
code takes from the same reasoning."""
import os

import numpy as np
import pytest

import group_model as model
import key_model
from oracle_lib import Oracle
from vectors import ED_B, L, P, ed_add, ed_enc, ed_mul

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_1024.npz")
NEUTRAL_ENC = (1).to_bytes(32, "little")


@pytest.fixture(scope="module")
def cases():
    sc, pt, labels = model.case_set()
    return sc, pt, labels


def test_case_set_has_every_scalar_with_every_label(cases):
    sc, pt, labels = cases
    want = {"base point", "honest", "honest negated", "mixed order", "small order", "y >= p", "x = 0 with the sign bit", "off the curve",
            "predicate boundary"}
    assert set(labels) == want
    scal = model.scalars()
    assert len(sc) == len(scal) * len(want) and 150 <= len(sc) <= 260
    for s in model.edge_scalars():
        assert {l for l, row in zip(labels, sc) if row.tobytes() == s} == want
    small = {p.tobytes() for p, l in zip(pt, labels) if l == "small order"}
    assert len(small) == 14, "every small-order encoding meets a scalar"


def test_fast_walk_is_ed_mul(cases):
    """the model's extended-coordinate walk against tests/vectors.py's affine one: one pair of every label, edge scalars first"""
    sc, pt, labels = cases
    seen = set()
    for s, p, lab in zip(sc, pt, labels):
        A = key_model.decode(p.tobytes())[0]
        e = model.scalar_value(s.tobytes(), False)
        if A is None or (lab, e > 8) in seen:
            continue
        seen.add((lab, e > 8))
        assert model.mul(e, A) == ed_mul(e, A), (lab, e)
    assert len(seen) >= 14
    assert model.mul(L, ED_B) == (0, 1) and model.mul(0, ED_B) == (0, 1)


def test_scalar_rule():
    for s in model.scalars():
        e = model.scalar_value(s, True)
        assert e % 8 == 0 and e >> 254 == 1
        assert model.scalar_value(s, False) == int.from_bytes(s, "little") % 2**255
    assert model.scalar_value(b"\xff" * 32, False) == 2**255 - 1
    assert model.scalar_value(bytes(31) + b"\x80", False) == 0, "bit 255 is ignored"


@pytest.mark.parametrize("w", model.WINDOWS)
def test_recoding_digit_counts(w):
    """129 / 86 / 65 digits hold every scalar below 2^255, every digit lies in [-R, R - 1] and the digits sum back; one digit fewer
    overflows at W = 2 (from 2^255 * 2/3: 2^254 + 2^253 and 2^255 - 1) and at W = 4 (from 2^255 * 14/15: 2^255 - 1)"""
    r, n = 1 << (w - 1), model.DIGITS[w]
    for s in model.scalars():
        for e in (model.scalar_value(s, True), model.scalar_value(s, False)):
            d = model.recode(e, w)
            assert len(d) == n and all(-r <= x < r for x in d)
            assert sum(x << (w * i) for i, x in enumerate(d)) == e
    c_short = sum(r << (w * i) for i in range(n - 1))
    for e in {2: (2**255 - 1, 2**254 + 2**253), 3: (), 4: (2**255 - 1,)}[w]:
        assert e + c_short >= 1 << (w * (n - 1)), "the obvious count is one short"


def test_pinned_to_the_reference_shared_secret():
    """for every decodable case point P and a clamped scalar s: u([s]P) == X25519(s, u(P)) by the compiled reference"""
    keys, labels = key_model.case_set()
    rng = np.random.default_rng(0x2551)
    pts = [k.tobytes() for k in keys if key_model.decode(k.tobytes())[0] is not None]
    assert len(pts) > 80
    sc = [key_model.clamp(rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in pts]
    u_in = np.stack([np.frombuffer(model.montgomery_u_of(p), np.uint8) for p in pts])
    want, _ = Oracle().x25519_shared(u_in, np.stack([np.frombuffer(s, np.uint8) for s in sc]))
    nonzero = 0
    for i, (s, p) in enumerate(zip(sc, pts)):
        q, ok = model.scalarmult(s, p, True)
        assert ok == 1
        assert model.montgomery_u_of(q) == want[i].tobytes(), (i, p.hex())
        nonzero += any(want[i])
    assert nonzero > 40, "honest and mixed-order points give a shared secret that is not zero"


def test_base_pinned_to_the_golden_public_keys():
    z = np.load(GOLDEN)
    for i in range(0, 1024, 16):
        s = model.seed_scalar(z["ed_sk"][i].tobytes())
        assert model.scalarmult_base(s, True) == model.scalarmult_base(s, False) == z["ed_pub"][i].tobytes(), i


def test_encoding_and_rejection(cases):
    sc, pt, labels = cases
    q, ok = model.expected_scalarmult(sc, pt, False)
    lab = np.array(labels)
    assert not ok[lab == "off the curve"].any() and not q[ok == 0].any()
    assert ok[lab == "honest"].all() and ok[lab == "mixed order"].all() and ok[lab == "small order"].all()
    zero = np.array([model.scalar_value(s.tobytes(), False) == 0 for s in sc])
    assert zero.any() and all(r.tobytes() == NEUTRAL_ENC for r in q[zero & (ok == 1)]), "[0]P is 01 00 .. 00 with ok = 1"
    for r in q[ok == 1]:
        assert int.from_bytes(r.tobytes(), "little") & key_model.MASK255 < P
    cq, cok = model.expected_scalarmult(sc, pt, True)
    assert np.array_equal(cok, ok)
    assert all(r.tobytes() == NEUTRAL_ENC for r in cq[(lab == "small order")]), "a clamped scalar kills every small-order point"


def test_group_laws():
    a, b = 0x1234567 * L // 7 % L, 0x7654321
    A, B = ed_enc(ed_mul(a, ED_B)), ed_enc(ed_mul(b, ED_B))
    assert model.point_add(A, B, False) == (ed_enc(ed_mul((a + b) % L, ED_B)), 1)
    assert model.point_add(A, B, True) == (ed_enc(ed_mul((a - b) % L, ED_B)), 1)
    assert model.point_add(A, A, True) == (NEUTRAL_ENC, 1)
    assert model.point_add(A, A, False) == (ed_enc(ed_add(ed_mul(a, ED_B), ed_mul(a, ED_B))), 1)
    assert model.scalarmult_base((L + 5).to_bytes(32, "little"), False) == model.scalarmult_base((5).to_bytes(32, "little"), False)
    p, q, names = model.add_cases()
    r, ok = model.expected_add(p, q, False)
    assert 0 < ok.sum() < len(ok) and not r[ok == 0].any()
    neg = np.array([n.endswith("P + (-P)") for n in names])
    assert all(x.tobytes() == NEUTRAL_ENC for x in r[neg & (ok == 1)])
