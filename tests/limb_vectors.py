"""Edge inputs for the raw-limb self-test hooks (include/curve25519_amd.h: c25519_amd_*_limb_selftest) and their big-integer
reference.  Every operand class comes from tools/fe_bounds.py -- the contract's limits (CONTRACT, at_beta), the reduced class
(reduced_fixpoint), FROM_WORDS, 2p (P2) -- so the bound proof and these tests cannot drift apart.  Shared by the CPU model's tests
(tests/test_field_limits.py) and the device's (tests/test_gpu_field_limits.py)."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fe_bounds as fb  # noqa: E402

P = 2**255 - 19
POS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
W, MASK, P2, U32 = fb.W, fb.MASK, fb.P2, fb.U32
IN_WORDS, OUT_WORDS = 84, 72                         # lanes.cuh: LIMB_IN_WORDS, LIMB_OUT_WORDS
R = fb.reduced_fixpoint()
FROM_WORDS = fb.FROM_WORDS
ZERO = [0] * 10
ALL_ONES = 0xFFFFFFFF


def value(limbs):
    return sum(int(x) << p for x, p in zip(limbs, POS))


def at(beta):
    return [min(x, U32) for x in fb.at_beta(beta)]


def canonical_limbs(v):
    """v (0 <= v < 2^256) in radix 2^25.5, limb 9 taking whatever is above 2^230."""
    out = []
    for i in range(9):
        out.append(v & MASK[i])
        v >>= W[i]
    return out + [v]


def inflated(v, bound):
    """Limbs below `bound` whose value is congruent to v mod p and as large as they can be: bound minus the canonical limbs of the
    difference, so most limbs sit at or just under their maximum."""
    d = (value(bound) - v) % P
    dl = canonical_limbs(d)
    assert all(b >= x for b, x in zip(bound, dl)), "bound below beta 1"
    return [b - x for b, x in zip(bound, dl)]


SPECIAL = [0, 1, 2, 19, P - 1, P, P + 1, P + 18, 2 * P - 1, 2 * P, 2**255 - 1, 2**255, 2**256 - 1] + \
          [2**255 - 19 + k for k in (-2, -1, 1, 2, 17, 18, 19, 20, 37, 38)]


def classes(bound, rng, n_random=24):
    """The operand vectors of one class: every limb at the bound, one limb at it with the rest zero, alternating max / zero,
    non-canonical representations of the special values inflated to the bound, seeded uniform limbs below the bound."""
    out = [list(bound)]
    for i in range(10):
        out.append([bound[j] if j == i else 0 for j in range(10)])
    out.append([bound[j] if j % 2 == 0 else 0 for j in range(10)])
    out.append([bound[j] if j % 2 == 1 else 0 for j in range(10)])
    for v in SPECIAL:
        out.append(inflated(v % P, bound))
        if v < 2**256:
            c = canonical_limbs(v)
            if all(x <= b for x, b in zip(c, bound)):
                out.append(c)
    for _ in range(n_random):
        out.append([rng.randrange(b + 1) for b in bound])
    for _ in range(n_random // 4):                                   # near the top of every limb at once
        out.append([b - rng.randrange(1 << 8) for b in bound])
    return out


def records(fields, ctl=0):
    """fields: up to eight limb vectors -> one input record (84 words)."""
    rec = np.zeros(IN_WORDS, np.uint32)
    for k, f in enumerate(fields):
        assert all(0 <= x <= U32 for x in f), f
        rec[10 * k: 10 * k + 10] = f
    rec[80] = ctl
    return rec


def pairs(ca, cb, rng, cap=None):
    """Every a with the worst b, the worst a with every b, and random pairings."""
    out = [(a, cb[0]) for a in ca] + [(ca[0], b) for b in cb[1:]]
    out += [(rng.choice(ca), rng.choice(cb)) for _ in range(len(ca))]
    return out if cap is None else out[:cap]


# ---- the big-integer reference -----------------------------------------------------------------------------------------------
def ref_ladder(SX, SZ, DX, DZ, base, eq, base9):
    """ecp_Mont as x25519.cuh's ladder_step computes it: S' = S + D (difference = base), D' = 2 (eq ? D : S)."""
    A, B, C, Dp = SX - SZ, SX + SZ, DX - DZ, DX + DZ
    Pd, M = (Dp, C) if eq else (B, A)
    DA, CB = A * Dp, C * B
    nSX = (DA + CB) ** 2
    nSZ = (DA - CB) ** 2 * (9 if base9 else base)
    AA, BB = Pd * Pd, M * M
    E = AA - BB
    return [x % P for x in (nSX, nSZ, AA * BB, E * (AA + 121665 * E))]


def ref_mont_double(X, Z):
    AA, BB = (X + Z) ** 2, (X - Z) ** 2
    E = AA - BB
    return [AA * BB % P, E * (AA + 121665 * E) % P]


def ref_double(X, Y, Z):
    """ge_double's formulas with its signs (Hn = A + B, Fn = 2 Z^2 + A - B): (X3, Y3, Z3, T3)."""
    A, B = X * X, Y * Y
    Hn, G = A + B, B - A
    E = (X + Y) ** 2 - Hn
    Fn = 2 * Z * Z + A - B
    return [x % P for x in (E * Fn, G * Hn, G * Fn, E * Hn)]


def ref_add(X, Y, Z, T, ypx, ymx, t2d, z2):
    """ge_add_pe (z2 given) / ge_add_pa (z2 = None: D = 2Z): (X3, Y3, Z3, T3)."""
    a, b, c = (Y - X) * ymx, (Y + X) * ypx, T * t2d
    d = 2 * Z if z2 is None else Z * z2
    e, h, f, g = b - a, b + a, d - c, d + c
    return [x % P for x in (e * f, g * h, f * g, e * h)]


def ref_lane(op, vals, ctl):
    """Expected values (mod p) of the four output elements of fe_limb_selftest_op (lanes.cuh)."""
    x, y, z = vals[0], vals[1], vals[2]
    if op in (14, 15):
        return ref_ladder(*vals[:5], ctl != 0, op == 15)
    if op == 16:
        return ref_double(vals[0], vals[1], vals[2])
    if op == 17:
        return ref_add(*vals[:7], None)
    if op == 18:
        return ref_add(*vals[:8])
    r = {0: x * y, 1: x * y, 2: x * x, 3: x * x, 4: x * x - y, 5: 2 * x * x + y - z, 6: x + 121665 * y, 7: 9 * x, 8: x, 9: x + y,
         10: x - y, 11: -x, 12: x}.get(op)
    if op == 13:
        r = pow(x, P - 2, P)
    return [r % P, 0, 0, 0]


def ref_quad(op, vals, ctl):
    """quad::limb_selftest_op: lanes (q0..q3) = (SX, SZ, DX, DZ) of a ladder step, (X, Y, T, Z) of a point."""
    if op in (0, 1):
        return ref_ladder(*vals[:5], ctl != 0, op == 1)
    X, Y, T, Z = vals[:4]
    if op == 2:
        X3, Y3, Z3, T3 = ref_add(X, Y, Z, T, vals[4], vals[5], vals[6], vals[7])
    else:
        X3, Y3, Z3, T3 = ref_double(X, Y, Z)
    return [X3, Y3, T3, Z3]


def ref_wave(op, vals, ctl):
    """coop::limb_selftest_op: rows 0..3."""
    if op == 0:
        return [vals[r] * vals[4 + r] % P for r in range(4)]
    if op == 1:
        return [(vals[r] + (vals[4 + r] << 32)) % P for r in range(4)]   # (the caller gives S; see wave_carry_value)
    if op in (2, 3):
        return ref_ladder(*vals[:5], ctl != 0, op == 3)
    if op == 4:
        return ref_mont_double(vals[0], vals[1]) + ref_mont_double(vals[2], vals[3])
    if op == 5:
        return ref_double(vals[0], vals[1], vals[2])
    X, Y, Z, T = vals[:4]
    ypx, ymx, t2d, z2 = vals[4:8]
    if ctl:
        ypx, ymx, t2d = ymx, ypx, -t2d
    return ref_add(X, Y, Z, T, ypx, ymx, t2d, z2)


# ---- the cases: (shape, op) -> input records ----------------------------------------------------------------------------------
LANE_OPS = {0: "fe_mul", 1: "fe_mul_runs", 2: "fe_sqr", 3: "fe_sqr_runs", 4: "fe_sqr_sub", 5: "fe_sqr2_add_sub", 6: "fe_mul121665_add",
            7: "fe_mul_small", 8: "fe_carry32", 9: "fe_add", 10: "fe_sub", 11: "fe_neg", 12: "fe_to_words", 13: "fe_invert",
            14: "ladder_step", 15: "ladder_step<BASE9>", 16: "ge_double", 17: "ge_add_pa", 18: "ge_add_pe"}
QUAD_OPS = {0: "quad::ladder_step", 1: "quad::ladder_step<BASE9>", 2: "quad::ge_add_fields", 3: "quad::ge_double"}
WAVE_OPS = {0: "coop::mul_level", 1: "coop::carry_small", 2: "coop::ladder_step", 3: "coop::ladder_step<BASE9>", 4: "coop::mont_double",
            5: "coop::ge_dbl", 6: "coop::ge_add_pe"}
# ops whose outputs the contract calls reduced (limbs <= reduced_fixpoint())
LANE_REDUCED = {0, 1, 2, 3, 4, 5, 6, 7, 8, 13, 14, 15, 16, 17, 18}
C = fb.CONTRACT


def lane_cases(op, scale=1.0, seed=0):
    """Input records of one-lane op `op`, operands at `scale` x the contract's documented maxima (scale > 1: the bite test)."""
    rng = random.Random(1000 * op + seed)
    s = lambda beta: at(beta * scale)  # noqa: E731
    recs = []
    if op in (0, 1):
        for a, b in pairs(classes(s(C["mul_a"]), rng), classes(s(C["mul_b"]), rng), rng):
            recs.append(records([a, b]))
        for a, b in ((R, R), (fb.add(R, R), fb.sub(R, R)), (fb.sub(R, R), fb.sub(R, R)), (fb.add(fb.sub(R, R), R), fb.sub(R, R))):
            recs.append(records([a, b]))                            # what callers pass: sums and differences of reduced values
    elif op in (2, 3):
        recs += [records([a]) for a in classes(s(C["sqr"]), rng)]
        recs += [records([a]) for a in (R, fb.add(R, R), fb.sub(R, R))]
    elif op == 4:
        for a, m in pairs(classes(s(C["sqr"]), rng), classes([2 * x for x in P2], rng), rng):
            recs.append(records([a, m]))
        recs.append(records([fb.add(R, R), fb.add(R, R)]))          # ge_double: (X+Y)^2 - (A+B)
    elif op == 5:
        for a, pm in pairs(classes(s(C["sqr2"]), rng), classes(P2, rng), rng):
            recs.append(records([a, at(C["small"]), pm]))
            recs.append(records([a, pm, P2]))
        recs.append(records([R, R, R]))                             # ge_double: 2 Z^2 + A - B
    elif op in (6, 7):
        for a, b in pairs(classes(s(C["small"]), rng), classes(s(C["small"]), rng), rng):
            recs.append(records([a, b]))
    elif op == 8:
        recs += [records([a]) for a in classes(s(C["carry32"]), rng)]
    elif op == 9:
        for a, b in pairs(classes(at(31), rng), classes(at(31), rng), rng):
            recs.append(records([a, b]))
    elif op == 10:
        for a, b in pairs(classes(at(C["mul_a"]), rng), classes(P2, rng), rng):
            recs.append(records([a, b]))
    elif op == 11:
        recs += [records([a]) for a in classes(P2, rng)]
    elif op == 12:
        for bound in (R, at(2), at(3), at(C["mul_a"]), at(8)):
            recs += [records([a]) for a in classes(bound, rng, 8)]
    elif op == 13:
        recs += [records([a]) for a in classes(R, rng, 8)]
    elif op in (14, 15):
        for st in classes(R, rng, 16):
            for eq in (0, ALL_ONES):
                recs.append(records([st, R, st, R, FROM_WORDS], eq))
                recs.append(records([R, st, R, st, classes(FROM_WORDS, rng, 0)[rng.randrange(10)]], eq))
        for eq in (0, ALL_ONES):
            recs.append(records([R, R, R, R, FROM_WORDS], eq))
    elif op == 16:
        for v in classes(R, rng, 16):
            recs.append(records([v, R, v, R]))
            recs.append(records([R, v, R, v]))
    else:
        t2d_neg = fb.select(fb.neg(R), R)                           # a row negated on the fly (beta 2)
        for v in classes(R, rng, 12):
            for q in ([R, R, t2d_neg, R], [FROM_WORDS, FROM_WORDS, P2, FROM_WORDS], [v, v, v, v]):
                recs.append(records([v, R, R, v] + q))
                recs.append(records([R, R, R, R] + q))
    return np.stack([r for r in recs if max(r[:80]) <= U32]).astype(np.uint32)


def quad_cases(op, seed=0):
    rng = random.Random(7000 + op + seed)
    recs = []
    if op in (0, 1):
        for st in classes(R, rng, 16):
            for eq in (0, ALL_ONES):
                recs.append(records([st, R, R, st, FROM_WORDS], eq))
                recs.append(records([R, st, st, R, rng.choice(classes(FROM_WORDS, rng, 4))], eq))
        for eq in (0, ALL_ONES):
            recs.append(records([R, R, R, R, FROM_WORDS], eq))
    elif op == 2:
        mult = fb.quad_mult_field()                                 # beta 2: a negated row field
        for v in classes(R, rng, 12):
            recs.append(records([v, R, R, v, FROM_WORDS, FROM_WORDS, mult, [2] + [0] * 9]))
            recs.append(records([R, R, R, R, mult, mult, mult, mult]))
            recs.append(records([R, v, v, R, v, mult, P2, mult]))
    else:
        for v in classes(R, rng, 16):
            recs.append(records([v, R, R, v]))
            recs.append(records([R, v, v, R]))
    return np.stack(recs).astype(np.uint32)


def wave_cases(op, seed=0):
    rng = random.Random(9000 + op + seed)
    recs = []
    if op == 0:
        for a, b in pairs(classes(at(C["mul_a"]), rng, 12), classes(at(C["mul_b"]), rng, 12), rng, cap=80):
            recs.append(records([a, R, R, a, b, b, R, P2]))
    elif op == 1:
        top = fb.CARRY_SMALL_IN - 1                                 # carry_small's precondition S < 2^46, as (low, high) words
        for S in classes([top] * 10, rng, 16)[:60]:
            S = [min(x, top) for x in S]
            lo, hi = [x & U32 for x in S], [x >> 32 for x in S]
            recs.append(records([lo, lo, lo, lo, hi, hi, hi, hi]))
    elif op in (2, 3):
        for st in classes(R, rng, 8)[:40]:
            for eq in (0, ALL_ONES):
                recs.append(records([st, R, R, st, FROM_WORDS], eq))
    elif op in (4, 5):
        for v in classes(R, rng, 8)[:40]:
            recs.append(records([v, R, R, v]))
    else:
        for v in classes(R, rng, 8)[:24]:
            for neg in (0, 1):
                recs.append(records([v, R, R, v, R, R, fb.select(fb.neg(R), R), R], neg))
                recs.append(records([R, v, v, R, P2, FROM_WORDS, P2, R], neg))
    return np.stack(recs).astype(np.uint32)


def values_in(recs):
    return [[value(r[10 * k: 10 * k + 10]) for k in range(8)] for r in recs]


def words_value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def check(shape, op, recs, out, reduced_bound=None, small_bound=None):
    """Value (mod p) of every output element and its canonical words; limb bounds where the contract names one.  Returns a list of
    failure messages (empty: all good)."""
    ref = {"lane": ref_lane, "quad": ref_quad, "wave": ref_wave}[shape]
    bad = []
    for i, (rec, o, vals) in enumerate(zip(recs, out, values_in(recs))):
        exp = ref(op, vals, int(rec[80]))
        for k in range(4):
            limbs = [int(x) for x in o[10 * k: 10 * k + 10]]
            got = value(limbs) % P
            words = words_value(o[40 + 8 * k: 48 + 8 * k])
            if got != exp[k]:
                bad.append(f"{shape} op {op} record {i} element {k}: value {got:#x} != {exp[k]:#x}")
            elif words != exp[k]:
                bad.append(f"{shape} op {op} record {i} element {k}: canonical words {words:#x} != {exp[k]:#x}")
            for bound, what in ((reduced_bound, "reduced"), (small_bound, "carry_small")):
                if bound is not None and any(x > b for x, b in zip(limbs, bound)):
                    bad.append(f"{shape} op {op} record {i} element {k}: limbs {limbs} above the {what} bound")
            if len(bad) > 20:
                return bad
    return bad


def wave_small_bound():
    """carry_small's output for any input meeting its precondition S < 2^46 (fe_bounds.carry_small)."""
    b = fb.carry_small([fb.CARRY_SMALL_IN - 1] * 10, "wave hook")
    fb.SMALL_SEEN.pop()
    return b
