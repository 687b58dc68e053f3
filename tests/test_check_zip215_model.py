"""The coset comparison of ed25519_Verify_Check_zip215_* (tests/check_zip215_model.py: no decoding of R) against the ZIP-215 rule as
stated (tests/zip215_cases.py: decode R, multiply by 8): the conformance grid, the torsion and degenerate sets and a generated set of
torsion-shifted R's in every encoding; and the closed form of the batch equation's point (tests/batch_eq_model.py: rows whose S is
moved by a known delta) against the slow models of the plain and the coalesced equation.  Big integers only."""
import random

import numpy as np

import batch_eq_indexed_model as im
import batch_eq_model as bm
import check_zip215_model as cm
import zip215_cases as zc
from vectors import D_ED, P, ed_add, ed_mul


def both(sig, pk, msg):
    """(rule as stated, coset comparison on affine T, coset comparison on (X : Y : Z) with a random Z)"""
    rnd = random.Random(len(sig))
    ref = zc.zip215_rule(sig, pk, msg)
    aff = cm.model_verdicts(sig, pk, msg)
    proj = np.array([cm.check_verdict(sig[i], pk[i], msg[i], z=rnd.randrange(2, P)) for i in range(len(sig))], np.int32)
    return ref, aff, proj


def test_constants():
    assert cm.SQRTM1 * cm.SQRTM1 % P == P - 1
    x8, y8 = cm.T8
    assert ed_mul(8, cm.T8) == (0, 1) and ed_mul(4, cm.T8) != (0, 1)
    assert (y8 * y8 - x8 * x8 - 1 - D_ED * x8 * x8 * y8 * y8) % P == 0
    assert cm.K8 == D_ED * x8 * y8 % P


def test_fast_mul_is_ed_mul():
    rnd = random.Random(216)
    from vectors import ED_B
    for k in (0, 1, 2, 8, rnd.getrandbits(253), rnd.getrandbits(256)):
        for pt in (ED_B, ed_add(ED_B, cm.torsion_points()[3]), cm.torsion_points()[5]):
            assert cm.fast_mul(k, pt) == ed_mul(k, pt)


def test_candidates_are_the_coset():
    """the projective algebra's eight candidates are T + t for the eight t, for random points and random Z"""
    rnd = random.Random(215)
    from vectors import ED_B
    for _ in range(8):
        T = ed_mul(rnd.getrandbits(252), ED_B)
        T = ed_add(T, cm.torsion_points()[rnd.randrange(8)])
        z = rnd.randrange(1, P)
        X, Y = T[0] * z % P, T[1] * z % P
        w_inv = pow(cm.coset_prep(X, Y, z), P - 2, P)
        cands = cm.coset_candidates(X, Y, z, w_inv)
        got = {c for c in cands} | {((P - x) % P, (P - y) % P) for x, y in cands}
        assert got == {ed_add(T, t) for t in cm.torsion_points()}


def test_conformance_grid():
    sig, pk, msg = zc.conformance_grid()
    assert len(sig) == 196
    ref, aff, proj = both(sig, pk, msg)
    assert ref.all() and aff.all() and proj.all()


def test_torsion_and_degenerate_sets():
    ref, aff, proj = both(*zc.torsion())
    assert ref.all() and aff.all() and proj.all()            # the cofactored rule accepts all eight shifts
    ref, aff, proj = both(*zc.degenerate()[:3])
    assert np.array_equal(aff, ref) and np.array_equal(proj, ref)
    assert ref.any() and not ref.all()


def test_generated_set():
    sig, pk, msg, labels = cm.generated_set()
    ref, aff, proj = both(sig, pk, msg)
    bad = [(i, labels[i], int(ref[i]), int(aff[i]), int(proj[i])) for i in range(len(sig)) if not ref[i] == aff[i] == proj[i]]
    assert not bad, bad[:10]
    by = {}
    for lab, v in zip(labels, ref):
        by.setdefault(lab, set()).add(int(v))
    assert by["valid"] == {1} and by["small_r_valid"] == {1} and by["small_r_small_key"] == {1}
    for lab in ("y_bit_flipped", "s_plus_1", "s_plus_l", "r_undecodable", "key_undecodable", "small_r_s_plus_1"):
        assert by[lab] == {0}, (lab, by[lab])
    assert by["sign_flipped"] <= {0, 1}                      # (a flipped sign bit on x = 0 still decodes to the same point)
    # every non-canonical encoding that exists is in the set
    vals = [int.from_bytes(bytes(s[:32]), "little") for s in sig]
    assert any((v & zc.MASK255) >= P for v in vals) and any(v >> 255 and (v & zc.MASK255) % P in (1, P - 1) for v in vals)


def test_zero_product_and_rule_2():
    sig, pk, msg = zc.conformance_grid()
    assert cm.coset_projective(0, 0, 0, bytes(32)) == 0       # Z = 0: the zero point a bad index leaves, R = 32 zero bytes
    assert cm.coset_projective(5, 7, 0, bytes(sig[0][:32])) == 0
    # row 1 of a context holds -A; a y without a square root leaves an x that is not on the curve whatever it is
    from vectors import ED_B
    A = ed_mul(12345, ED_B)
    nx = (P - A[0]) % P
    assert cm.key_on_curve_from_row1((A[1] + nx) % P, (A[1] - nx) % P, A[1]) == 1
    assert cm.key_on_curve_from_row1((A[1] + nx + 1) % P, (A[1] - nx) % P, A[1]) == 0
    assert cm.key_on_curve_from_row1((A[1] + nx) % P, (A[1] - nx) % P, (A[1] + 1) % P) == 0


# ---- the batch equation's closed form against its slow models ---------------------------------------------------------------

def _shifted_dozen(oracle):
    """12 rows: 9 honest ones (exactly valid, cofactorless) with S moved, one of them then rejected, and 3 torsion rows under one
    mixed-order key at rows 2, 5, 11: (sig, pk, msg, special rows, shifted rows that stay, their deltas)"""
    pub, priv = oracle.ed25519_keypair(oracle.random_bytes((12, 32), 0xC105ED))
    msg = oracle.random_bytes((12, 32), 0xC105EE)
    sig = oracle.ed25519_sign(priv, msg).copy()
    assert oracle.ed25519_verify(sig, pub, msg).all()
    tsig, tpk, tmsg = zc.torsion()
    special = [2, 5, 11]
    sig[special], pub[special], msg[special] = tsig[:3], tpk[:3], tmsg[:3]
    assert len({bytes(k) for k in tpk[:3]}) == 1
    rows = [i for i in range(12) if i not in special]
    deltas = bm.odd_deltas(len(rows), 0xC105EF)
    sig = bm.shift_s(sig, rows, deltas)
    sig[7, 32:] = np.frombuffer(bm.L.to_bytes(32, "little"), np.uint8)            # S = L: the row drops out, its delta with it
    kept = [(r, d) for r, d in zip(rows, deltas) if r != 7]
    return sig, pub, msg, special, [r for r, _ in kept], [d for _, d in kept]


def test_closed_form_of_the_batch_point_equals_the_slow_model(oracle):
    sig, pk, msg, special, rows, deltas = _shifted_dozen(oracle)
    seed = bytes(range(32))
    sums = bm.shift_sums(seed, rows, deltas)
    share = bm.subset_points(sig[special], pk[special], msg[special], seed, special, (3, 6, 12))
    for n in (3, 6, 12):
        want, ok = bm.batch_point(sig[:n], pk[:n], msg[:n], seed)
        assert ok == (n <= 7) and bm.shifted_point(sums, n, share[n]) == want, n
    assert bm._affine(share[12]) == bm.batch_point(sig[special], pk[special], msg[special], seed, index=special)[0]
    # steering: row 9's delta replaced, then row 5's (a special row) moved as well -- the sum is zero, T the special rows' share
    for j in (9, 5):
        d = bm.steering_delta(seed, sums, 12, j)
        base = sig if j in special else bm.shift_s(sig, [j], [-deltas[rows.index(j)]])
        steered = bm.shift_s(base, [j], [d])
        want, _ = bm.batch_point(steered, pk, msg, seed)
        assert want == bm._affine(share[12]) and bm._affine(bm._mul(8, bm._ext(want))) == (0, 1), j
        assert zc.zip215_rule(steered[[0, j]], pk[[0, j]], msg[[0, j]]).tolist() == [0, 0]


def test_closed_form_of_the_coalesced_point_equals_the_slow_model(oracle):
    sig, pk, msg, special, rows, deltas = _shifted_dozen(oracle)
    seed = bytes(range(32, 64))
    keys, idx = im.distinct_keys(pk)
    assert len(keys) == 10
    sp = np.array(special)
    share, _ = im.batch_point(keys, idx[sp], sig[sp], msg[sp], seed, index=sp)
    want, ok = im.batch_point(keys, idx, sig, msg, seed)
    assert not ok and bm.shifted_point(bm.shift_sums(seed, rows, deltas), 12, bm._ext(share)) == want
