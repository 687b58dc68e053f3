"""tests/msm_model.py (the yardstick of the multiscalar calls) against the two models it stands on: a group's sum by the pooled
big-integer formula equals the chain a caller composes today, scalarmult then point_add row by row, in tests/group_model.py and
tests/ristretto_model.py.  Tiny cases only: the chain walks every row."""
import numpy as np
import pytest

import group_model
import msm_model as model
import ristretto_model
from vectors import L


def _composed(group, sc, pt, m):
    """the chain per group: [s_i mod L] P_i by the group's scalarmult (the reduced scalar is below 2^255, so its low 255 bits are the
    scalar), then point_add from the left"""
    mult = (lambda s, p: group_model.scalarmult(s, p, False)) if group == "ed25519" else ristretto_model.scalarmult
    add = group_model.point_add if group == "ed25519" else ristretto_model.point_add
    q, ok = [], []
    for g in range(0, len(sc), m):
        acc, good = model.IDENTITY[group], 1
        for s, p in zip(sc[g:g + m], pt[g:g + m]):
            r, k = mult(model._le(int.from_bytes(bytes(s), "little") % L), bytes(p))
            good &= k
            if good:
                acc = add(acc, r, False)[0]
        q.append(acc if good else model.ZERO32)
        ok.append(good)
    return model._rows(q), np.array(ok, np.int32)


@pytest.mark.parametrize("group", model.GROUPS)
@pytest.mark.parametrize("shape", ((1, 1), (1, 2), (3, 1), (2, 5), (1, 40)))
def test_the_pooled_sum_is_the_composed_chain(group, shape):
    n_groups, m = shape
    sc, pt = model.case(group, n_groups, m, seed=3)
    q, ok = model.expected(group, sc, pt, m)
    cq, cok = _composed(group, sc, pt, m)
    assert np.array_equal(ok, cok) and ok.all()
    assert np.array_equal(q, cq)


@pytest.mark.parametrize("group", model.GROUPS)
def test_equal_scalars_and_cancelling_groups(group):
    sc, pt = model.case(group, 2, 6, seed=5, kind="equal")
    assert np.array_equal(model.expected(group, sc, pt, 6)[0], _composed(group, sc, pt, 6)[0])
    sc, pt = model.case(group, 3, 4, seed=5, kind="cancel")
    q, ok = model.expected(group, sc, pt, 4)
    assert ok.all() and all(bytes(r) == model.IDENTITY[group] for r in q)
    assert np.array_equal(q, _composed(group, sc, pt, 4)[0])


@pytest.mark.parametrize("group", model.GROUPS)
def test_a_reject_zeroes_its_group_only(group):
    sc, pt = model.case(group, 3, 4, seed=7)
    clean = model.expected(group, sc, pt, 4)
    for which in ("non-decoding",) + (("non-canonical",) if group == "ristretto255" else ()):
        for row, g in ((11, 2), (0, 0)):
            q, ok = model.expected(group, sc, model.with_reject(group, pt, row, which), 4)
            assert ok.tolist() == [0 if i == g else 1 for i in range(3)]
            assert bytes(q[g]) == model.ZERO32
            assert all(np.array_equal(q[i], clean[0][i]) for i in range(3) if i != g)


def test_the_scalar_is_read_mod_l_on_the_mixed_order_point():
    """[L + 1]P is P + [L]P, a different point where P has a torsion part; the calls' rule is [(L + 1) mod L]P = P"""
    good, _ = model.pool("ed25519")
    mixed = good[11]
    assert group_model.scalarmult(model._le(L), mixed, False)[0] != model.IDENTITY["ed25519"], "the pool's mixed-order point has a torsion part"
    q, ok = model.expected_group("ed25519", [model._le(L + 1)], [mixed])
    assert ok == 1 and q == mixed
    assert q != group_model.scalarmult(model._le(L + 1), mixed, False)[0]
    q, ok = model.expected_group("ed25519", [model._le(L - 1), model._le(2)], [mixed, mixed])       # the inner sum L + 1 is an integer
    assert q == group_model.scalarmult(model._le(L + 1), mixed, False)[0]


def test_the_pool_and_the_scalar_sets_are_what_the_issue_lists():
    for group in model.GROUPS:
        good, rejects = model.pool(group)
        assert len(set(good)) == len(good) and len(good) + len(rejects) <= 16
        assert model.IDENTITY[group] in good
    for c in model.WIDTHS:
        zero, half, ones = (int.from_bytes(s, "little") for s in model.window_scalars(c))
        assert zero == 0 and max(half, ones) < L
        for w in range(252 // c):
            assert (half >> (c * w)) & ((1 << c) - 1) == 1 << (c - 1) and (ones >> (c * w)) & ((1 << c) - 1) == (1 << c) - 1
    assert set(model.EDGE_SCALARS) <= set(model.scalar_set(1))
