#!/usr/bin/env python3
"""Worst-case limb-bound checker for curve25519_amd/csrc/fe25519.cuh and every formula built on it.

The device field code keeps ten unsaturated limbs (radix 2^25.5) in 32-bit registers and 64-bit column
accumulators; it is only correct if no 32-bit operand, no 64-bit column and no biased subtraction ever
overflows / goes negative -- for ALL inputs, not just the random ones the parity tests throw at it.  This
script replays the formulas of x25519.cuh / ge25519.cuh / engine.hip, and those of the four-lane (quad25519.cuh) and
one-wave (coop25519.cuh) shapes, on per-limb upper bounds (interval arithmetic with exact Python integers; a per-lane
choice is the larger of its two sides) and asserts every such condition, starting from the worst inputs the contract
allows ("reduced" = whatever a mul/sqr carry chain, of either shape, can emit).  coop25519.cuh's carry_small has an output
class of its own (coop_small_class), checked at each of its consumers.  tests/limb_vectors.py builds the edge inputs of
the raw-limb tests from CONTRACT and these classes.  Run: python tools/fe_bounds.py
"""
M26, M25 = (1 << 26) - 1, (1 << 25) - 1
W = [26, 25] * 5
MASK = [M26, M25] * 5
P2 = [0x7FFFFDA] + [0x3FFFFFE, 0x7FFFFFE] * 4 + [0x3FFFFFE]
U32, U64 = (1 << 32) - 1, (1 << 64) - 1


class Bad(AssertionError):
    pass


def need(cond, what):
    if not cond:
        raise Bad(what)


def carry64(h, where):
    h = list(h)
    for i in range(10):
        need(h[i] <= U64, f"{where}: column {i} overflows 64 bits ({h[i].bit_length()} bits)")
    for i in range(9):
        h[i + 1] += h[i] >> W[i]
        need(h[i + 1] <= U64, f"{where}: carry into column {i+1} overflows")
        h[i] = min(h[i], MASK[i])
    c = h[9] >> 25
    h[9] = min(h[9], M25)
    h[0] += c * 19
    need(h[0] <= U64, f"{where}: wrap overflows")
    h[1] += h[0] >> 26
    h[0] = min(h[0], M26)
    need(all(x <= U32 for x in h), f"{where}: limb exceeds 32 bits after carry")
    return h


def mul(a, b, where="mul"):
    b19 = [19 * x for x in b]
    a2 = [2 * x for x in a]
    need(all(x <= U32 for x in b19[1:]), f"{where}: 19*b overflows 32 bits (max beta_b {max(b[i] / (1 << W[i]) for i in range(10)):.2f})")
    need(all(a2[i] <= U32 for i in range(1, 10, 2)), f"{where}: 2*a overflows 32 bits")
    h = [0] * 10
    for k in range(10):
        for i in range(10):
            j = (k - i) % 10
            x = a2[i] if (i & 1 and j & 1) else a[i]
            y = b19[j] if i > k else b[j]
            h[k] += x * y
    return carry64(h, where)


def sqr_columns(a, where):
    f2 = [2 * x for x in a]
    f19 = [19 * x for x in a]
    f38 = [38 * x for x in a]
    need(all(x <= U32 for x in f2), f"{where}: 2*a overflows")
    need(all(f19[j] <= U32 for j in range(5, 10)), f"{where}: 19*a overflows")
    need(all(f38[j] <= U32 for j in (5, 7, 9)), f"{where}: 38*a overflows (beta {a[9] / (1 << 25):.2f})")
    h = [0] * 10
    for k in range(10):
        for i in range(10):
            j = (k - i) % 10
            if i > j:
                continue
            wrap = i + j >= 10
            odd2 = i & 1 and j & 1
            if wrap and j & 1:
                x = f2[i] if (i < j and i & 1) else a[i]
                y = f38[j]
            else:
                x = f2[i] if i < j else a[i]
                y = f19[j] if wrap else (f2[j] if odd2 else a[j])
            h[k] += x * y
    return h


def sqr(a, where="sqr"):
    return carry64(sqr_columns(a, where), where)


def sqr_sub(a, m, where="sqr_sub"):
    h = sqr_columns(a, where)
    for i in range(10):
        need(m[i] <= 2 * P2[i], f"{where}: 4p bias smaller than subtrahend limb {i}")
        h[i] += 2 * P2[i]                       # upper bound of 4p - m is 4p
    return carry64(h, where)


def sqr2_add_sub(a, p, m, where="sqr2_add_sub"):
    h = sqr_columns(a, where)
    for i in range(10):
        need(m[i] <= P2[i], f"{where}: 2p bias smaller than subtrahend limb {i}")
        need(p[i] + P2[i] <= U32, f"{where}: 32-bit addend overflows")
        h[i] = 2 * h[i] + p[i] + P2[i]
    return carry64(h, where)


def chained_small_mul(mulitplicand, c, addend, where):
    """fe_mul121665_add / fe_mul_small: one MAD per limb, the previous limb's carry added to the 32-bit addend."""
    l, carry = [0] * 10, 0
    for i in range(10):
        t = addend[i] + carry
        need(t <= U32, f"{where}: addend + carry overflows 32 bits at limb {i}")
        h = mulitplicand[i] * c + t
        need(h <= U64, f"{where}: limb {i} overflows 64 bits")
        carry = h >> W[i]
        need(carry <= U32, f"{where}: carry out of limb {i} exceeds 32 bits")
        l[i] = min(h, MASK[i])
    t = l[0] + 19 * carry
    need(19 * carry <= U32 and t <= U32, f"{where}: wrap overflows 32 bits")
    l[1] += t >> 26
    l[0] = min(t, M26)
    need(all(x <= U32 for x in l), f"{where}: limb exceeds 32 bits")
    return l


def mul121665_add(a, b, where="mul121665_add"):
    return chained_small_mul(b, 121665, a, where)


def add(a, b, where="add"):
    r = [x + y for x, y in zip(a, b)]
    need(all(x <= U32 for x in r), f"{where}: 32-bit overflow")
    return r


def sub(a, b, where="sub"):
    need(all(b[i] <= P2[i] for i in range(10)), f"{where}: subtrahend limb exceeds 2p (would go negative)")
    r = [a[i] + P2[i] for i in range(10)]
    need(all(x <= U32 for x in r), f"{where}: 32-bit overflow")
    return r


def neg(a, where="neg"):
    need(all(a[i] <= P2[i] for i in range(10)), f"{where}: operand exceeds 2p")
    return list(P2)


def carry32(a, where="carry32"):
    h = list(a)
    for i in range(9):
        h[i + 1] += h[i] >> W[i]
        need(h[i + 1] <= U32, f"{where}: 32-bit overflow")
        h[i] = min(h[i], MASK[i])
    c = h[9] >> 25
    h[9] = min(h[9], M25)
    h[0] += 19 * c
    need(h[0] <= U32, f"{where}: 32-bit overflow")
    h[1] += h[0] >> 26
    h[0] = min(h[0], M26)
    return h


def to_words(a, where="to_words"):
    h = list(a)
    for _ in range(2):
        for i in range(9):
            h[i + 1] += h[i] >> W[i]
            need(h[i + 1] <= U32, f"{where}: 32-bit overflow")
            h[i] = min(h[i], MASK[i])
        c = h[9] >> 25
        h[9] = min(h[9], M25)
        h[0] += 19 * c
        need(h[0] <= U32, f"{where}: 32-bit overflow")
    need(h[0] <= M26 + 19, f"{where}: limb 0 not within 2^26+19 after two passes ({h[0]})")
    need(all(h[i] <= MASK[i] for i in range(1, 10)), f"{where}: limbs not strictly reduced after two passes")


def select(a, b):
    return [max(x, y) for x, y in zip(a, b)]


FROM_WORDS = [M26 + 19, M25, M26, M25, M26, M25, M26, M25, M26, M25]
ONE = [1] + [0] * 9
CANON = list(MASK)


# the documented operand limits of fe25519.cuh's contract, as beta = limb / 2^w (tests/limb_vectors.py builds its edge inputs from
# these too, so the proof and the tests cannot drift apart)
CONTRACT = {
    "mul_a": 5, "mul_b": 3.3,          # fe_mul
    "sqr": 3.3,                        # fe_sqr, fe_sqr_sub's a
    "sqr_sub_m": 2,                    # fe_sqr_sub's m (bias 4p)
    "sqr2": 2.3,                       # fe_sqr2_add_sub's a (columns doubled)
    "small": 7.9,                      # fe_mul121665_add, fe_mul_small: any beta < 8
    "carry32": 63,                     # fe_carry32: any beta < 2^6
}


def at_beta(beta):
    """Every limb at beta * 2^w (the largest limb vector of that class)."""
    return [int(beta * (1 << W[i])) for i in range(10)]


def reduced_fixpoint():
    """Largest limbs any carry chain can emit, iterated until stable."""
    red = list(FROM_WORDS)
    for _ in range(4):
        worst_in_a = at_beta(CONTRACT["mul_a"])
        worst_in_b = at_beta(CONTRACT["mul_b"])
        cands = [mul(worst_in_a, worst_in_b, "contract mul"), sqr(at_beta(CONTRACT["sqr"]), "contract sqr"),
                 carry32(at_beta(CONTRACT["carry32"]), "contract carry32"),
                 mul121665_add(at_beta(CONTRACT["small"]), at_beta(CONTRACT["small"]), "contract a24"),
                 chained_small_mul(at_beta(CONTRACT["small"]), 9, [0] * 10, "contract mul_small"),
                 # coop25519.cuh's product: its last carry pass leaves limbs up to 2^w + 1 (fe25519.cuh's chain masks them exactly)
                 coop_carry(coop_columns(worst_in_a, worst_in_b, "contract coop product"), "contract coop product")]
        new = [max([red[i]] + [c[i] for c in cands]) for i in range(10)]
        if new == red:
            break
        red = new
    return red


def beta(a):
    return max(a[i] / (1 << W[i]) for i in range(10))


def chain250(x, R):
    """fe_chain250 / fe_invert / fe_pow2523: every intermediate is a mul/sqr output, i.e. reduced."""
    x2 = sqr(x, "chain x2")
    t = sqr(sqr(x2, "c"), "c")
    x9 = mul(t, x, "chain x9")
    x11 = mul(x9, x2, "chain x11")
    for v in (x2, x9, x11):
        need(all(v[i] <= R[i] for i in range(10)), "chain output not reduced")
    # the remaining steps only combine reduced values
    mul(R, R, "chain mul")
    sqr(R, "chain sqr")
    mul(R, x, "chain final mul by x")
    return R


# ---- quad25519.cuh: four lanes per element; every per-lane choice (q_sel, a role mask) is a select ----------------------------
def quad_ladder_step(own, x1, base9, deeper=0):
    """quad::ladder_step on `own` (every lane's), x1 the base point's x.  deeper: extra q_sub levels on the level-2 operands
    (the bite test's knob)."""
    s, d = add(own, own, "quad l1 sum"), sub(own, own, "quad l1 diff")
    give, keep = select(d, s), select(s, d)
    got = give
    a, b = select(keep, got), select(keep, got)
    p = mul(a, b, "quad level 1")
    other = p
    s, d = add(p, other, "quad l2 sum"), sub(p, other, "quad l2 diff")
    keep = neg(other, "quad l2 -AA")
    got = mul121665_add(keep, d, "quad l2 a24")
    give = select(s, d)
    a = select(p, give)
    b = select(other, select(got, give))
    for _ in range(deeper):
        a, b = sub(a, R_QUAD, "deeper"), sub(b, R_QUAD, "deeper")
    p = mul(a, b, "quad level 2")
    a = chained_small_mul(p, 9, [0] * 10, "quad level 3 (times 9)") if base9 else mul(p, x1, "quad level 3")
    return select(a, p)


def quad_mult_field():
    """The `mult` of ge_add_fields: a row field from words or the LDS comb, negated by q_neg on q2 (beta 2), or the constant 2."""
    f = FROM_WORDS
    return select(select(neg(f, "row_field_unpack q_neg"), f), [2] + [0] * 9)


def quad_ge_add_fields(own, mult):
    s, d = add(own, own, "quad add Y+X"), sub(own, own, "quad add Y-X")
    a = select(d, select(s, own))
    p = mul(a, mult, "quad add level 1")
    s, d = add(p, p, "quad add h, g"), sub(p, p, "quad add e, f")
    a = select(s, select(d, d))
    b = select(d, select(s, s))
    return mul(a, b, "quad add level 2")


def quad_ge_double(own):
    s = add(own, own, "quad dbl X+Y")
    p = sqr(select(s, own), "quad dbl level 1")
    s, d = add(p, p, "quad dbl Hn"), sub(p, p, "quad dbl G")
    F = select(d, s)
    need(all(F[i] <= 2 * P2[i] for i in range(10)), "quad dbl: 4p bias smaller than the subtrahend")
    u = [p[i] + p[i] + 2 * P2[i] for i in range(10)]      # p + (p & is3) + 4p - F
    need(all(x <= U32 for x in u), "quad dbl: u overflows 32 bits")
    u = carry32(u, "quad dbl u")
    a = select(u, select(d, F))
    b = select(u, select(s, u))
    return mul(a, b, "quad dbl level 2")


# ---- coop25519.cuh: a field element limb per lane, a product as one column per lane -------------------------------------------
def coop_put_y(b, where):
    """put_y: the multiplier pre-scaled in 32 bits -- yo = 19 b, ye = 38 b for an odd limb, 19 b for an even one."""
    for j in range(10):
        need(19 * b[j] <= U32, f"{where}: 19*b overflows 32 bits (limb {j})")
        need((19 * b[j]) << (j & 1) <= U32, f"{where}: 38*b overflows 32 bits (limb {j})")
        need(b[j] << (j & 1) <= U32, f"{where}: 2*b overflows 32 bits (limb {j})")


def coop_columns(a, b, where):
    """coop::column: lane c's ten-term sum a_(9-t) * (yo or ye)[c+1+t]."""
    coop_put_y(b, where)
    yo = [19 * x for x in b] + list(b)
    ye = [(19 * b[j]) << (j & 1) for j in range(10)] + [b[j] << (j & 1) for j in range(10)]
    S = []
    for c in range(10):
        acc = sum(a[9 - t] * (yo[c + 1 + t] if t & 1 else ye[c + 1 + t]) for t in range(10))
        need(acc <= U64, f"{where}: column {c} overflows 64 bits")
        S.append(acc)
    return S


def coop_carry(S, where):
    """coop::carry / carry_packed (row_carry): S = l0 + 2^w l1 + 2^51 l2, limb_c = l0_c + l1_(c-1) + l2_(c-2) (19 x around the
    wrap), then one more pass of the bits above w."""
    need(all(x <= U64 for x in S), f"{where}: column sum overflows 64 bits")
    l0 = [min(S[c], MASK[c]) for c in range(10)]
    l1 = [min(S[c] >> W[c], MASK[(c + 1) % 10]) for c in range(10)]
    l2 = [S[c] >> 51 for c in range(10)]
    limb = []
    for c in range(10):
        x = l0[c] + (l1[c - 1] if c >= 1 else 19 * l1[9]) + (l2[c - 2] if c >= 2 else 19 * l2[c + 8])
        need(x <= U32, f"{where}: carried limb {c} overflows 32 bits")
        limb.append(x)
    e = [limb[c] >> W[c] for c in range(10)]
    out = [min(limb[c], MASK[c]) + (e[c - 1] if c else 19 * e[9]) for c in range(10)]
    need(all(x <= U32 for x in out), f"{where}: limb exceeds 32 bits")
    return out


CARRY_SMALL_IN = 1 << 46


def carry_small(S, where):
    """coop::carry_small: one piece moves up.  Precondition S < 2^46; out_c = (S_c & mask) + (S_(c-1) >> w), 19 x at the wrap."""
    need(all(x < CARRY_SMALL_IN for x in S), f"{where}: carry_small input reaches 2^46")
    out = [min(S[c], MASK[c]) + ((S[c - 1] >> W[c - 1]) if c else 19 * (S[9] >> 25)) for c in range(10)]
    need(all(x <= U32 for x in out), f"{where}: carry_small limb exceeds 32 bits")
    SMALL_SEEN.append(out)
    return out


SMALL_SEEN = []


def mul_level(a, b, where):
    return coop_carry(coop_columns(a, b, where), where)


def coop_small_class():
    """The named limb class of carry_small's outputs: the largest each limb reaches over every call site replayed so far."""
    return [max(v[i] for v in SMALL_SEEN) for i in range(10)]


def coop_ladder_step(v, x1, base9):
    val = select(sub(v, v, "coop ladder diff"), add(v, v, "coop ladder sum"))
    v = mul_level(val, val, "coop ladder level 1")                     # A Dp, C B, P^2, M^2 (sel is one of val's rows)
    d2 = sub(v, v, "coop ladder d2")
    base = select(d2, select(v, add(v, v, "coop ladder DA+CB")))
    w = carry_small(select([x * 121665 + y for x, y in zip(d2, v)], base), "coop ladder phase 1.5")
    x = select(v, w)
    v = mul_level(x, x, "coop ladder level 2")
    if base9:
        return coop_carry([9 * y for y in v], "coop ladder times 9 (carry_packed)")
    return mul_level(v, select(ONE, x1), "coop ladder level 3")


def coop_mont_double(v):
    val = select(sub(v, v, "coop dbl x-z"), add(v, v, "coop dbl x+z"))
    v = mul_level(val, val, "coop dbl level 1")
    E = sub(v, v, "coop dbl E")
    F = carry_small([x * 121665 + y for x, y in zip(E, v)], "coop dbl F")
    return mul_level(select(E, v), select(F, v), "coop dbl level 2")


def coop_ladder2(v):
    """ladder2_step_sum (wave 0) and ladder2_step_double (wave 1)."""
    val = select(sub(v, v, "coop2 sum A"), add(v, v, "coop2 sum B"))
    p = mul_level(val, val, "coop2 sum level 1")
    w = carry_small(select(add(p, p, "coop2 V"), sub(p, p, "coop2 U")), "coop2 sum V, U")
    s = mul_level(w, w, "coop2 sum level 2")
    return s, coop_mont_double(v)


def coop_ge_add_finish(v):
    w = select(add(v, v, "coop add h, g"), sub(v, v, "coop add e, f"))
    return mul_level(w, w, "coop add level 2")


def coop_ge_add(v, q):
    op = select(select(v, add(v, v, "coop add 2Z, Y+X")), sub(v, v, "coop add Y-X"))
    return coop_ge_add_finish(mul_level(op, select(q, ONE), "coop add level 1"))


def coop_ge_add_pe(v, q):
    t = select(neg(v, "coop add_pe -T"), v)
    op = select(select(t, add(v, v, "coop add_pe Y+X")), sub(v, v, "coop add_pe Y-X"))
    return coop_ge_add_finish(mul_level(op, q, "coop add_pe level 1"))


def coop_ge_dbl(v):
    x = select(v, add(v, v, "coop dbl X+Y"))
    p = mul_level(x, x, "coop ge_dbl level 1")
    hg = select(sub(p, p, "coop ge_dbl G"), add(p, p, "coop ge_dbl Hn"))
    need(all(hg[i] <= 2 * P2[i] for i in range(10)), "coop ge_dbl: 4p bias smaller than the subtrahend")
    up = [2 * p[i] + 2 * P2[i] for i in range(10)]
    need(all(y <= U32 for y in up), "coop ge_dbl: 2 Z^2 + 4p overflows 32 bits")
    w = carry_small(select(up, hg), "coop ge_dbl E, Fn")
    return mul_level(w, w, "coop ge_dbl level 2")


def quad_section(R):
    for base9 in (False, True):
        need(all(x <= r for x, r in zip(quad_ladder_step(R, FROM_WORDS, base9), R)), "quad ladder output not reduced")
    need(all(x <= r for x, r in zip(quad_ge_add_fields(R, quad_mult_field()), R)), "quad addition output not reduced")
    need(all(x <= r for x, r in zip(quad_ge_double(R), R)), "quad doubling output not reduced")
    # engine_common.cuh: the shared inversion's quad exchange -- pair = acc * partner, total = pair * other pair, then 1/total times both
    pair = mul(R, R, "batch invert pair")
    total = mul(pair, pair, "batch invert total")
    inv = mul(mul(R, pair, "batch invert x other pair"), R, "batch invert x partner")
    for v in (pair, total, inv):
        need(all(x <= r for x, r in zip(v, R)), "batch invert output not reduced")


def coop_section(R):
    del SMALL_SEEN[:]
    outs = [coop_ladder_step(R, FROM_WORDS, False), coop_ladder_step(R, FROM_WORDS, True), coop_mont_double(R), *coop_ladder2(R),
            coop_ge_add(R, select(P2, FROM_WORDS)), coop_ge_add_pe(R, select(R, P2)), coop_ge_dbl(R)]
    for v in outs:
        need(all(x <= r for x, r in zip(v, R)), "coop output not reduced: loop invariant broken")
    small = coop_small_class()
    # every consumer of a carry_small output is a product operand, first or second (put_a and put_y): within the contract
    need(all(small[i] <= at_beta(CONTRACT["mul_b"])[i] for i in range(10)), "carry_small output too large for a product operand")
    mul_level(small, small, "carry_small output as both factors")
    return small


R_QUAD = reduced_fixpoint()


def main():
    R = reduced_fixpoint()
    print(f"reduced limb bound: beta <= {beta(R):.6f}  (limb1 <= 2^25 + {R[1] - (1 << 25)})")
    need(all(R[i] <= P2[i] for i in range(10)), "reduced value exceeds 2p: fe_sub bias too small")

    # ---- x25519.cuh ----
    X1 = FROM_WORDS
    SX, SZ, DX, DZ = R, select(R, ONE), R, R

    def ladder_step(SX, SZ, DX, DZ):
        A = sub(SX, SZ, "ladder A")
        B = add(SX, SZ)
        C = sub(DX, DZ, "ladder C")
        Dp = add(DX, DZ)
        P, M = select(Dp, B), select(C, A)
        A = mul(A, Dp, "ladder A*D")
        B = mul(C, B, "ladder C*B")
        C = add(A, B)
        B = sub(A, B, "ladder A-B")
        nSX = sqr(C, "ladder x3")
        A = sqr(B, "ladder (A-B)^2")
        nSZ = mul(A, X1, "ladder z3")
        nSZ9 = chained_small_mul(A, 9, [0] * 10, "ladder z3, base point u = 9 (fe_mul_small)")
        need(all(nSZ9[i] <= R[i] for i in range(10)), "fe_mul_small output not reduced")
        A = sqr(P, "ladder AA")
        B = sqr(M, "ladder BB")
        nDX = mul(A, B, "ladder x4")
        B = sub(A, B, "ladder E")
        A = mul121665_add(A, B, "ladder a24")
        nDZ = mul(B, A, "ladder z4")
        return nSX, nSZ, nDX, nDZ

    out = ladder_step(SX, SZ, DX, DZ)
    for v in out:
        need(all(v[i] <= R[i] for i in range(10)), "ladder output not reduced: loop invariant broken")
    chain250(R, R)
    to_words(mul(R, R, "x25519 final"), "x25519 to_words")
    print("x25519 ladder, inversion, encoding: ok")

    # ---- ge25519.cuh ----
    def ge_double(X, Y, Z):
        A, B = sqr(X, "dbl A"), sqr(Y, "dbl B")
        Hn = add(A, B)
        G = sub(B, A, "dbl G")
        t = add(X, Y)
        E = sqr_sub(t, Hn, "dbl E")
        Fn = sqr2_add_sub(Z, A, B, "dbl Fn")
        return mul(E, Fn, "dbl X"), mul(G, Hn, "dbl Y"), mul(G, Fn, "dbl Z"), mul(E, Hn, "dbl T")

    def ge_add(X, Y, Z, T, ypx, ymx, t2d, z2):
        a = mul(sub(Y, X, "add Y-X"), ymx, "add a")
        b = mul(add(Y, X), ypx, "add b")
        c = mul(T, t2d, "add c")
        d = add(Z, Z) if z2 is None else mul(Z, z2, "add d")
        e, h = sub(b, a, "add e"), add(b, a)
        f, g = sub(d, c, "add f"), add(d, c)
        if z2 is None:      # ge_add_pa operand order
            return mul(f, e, "add X"), mul(g, h, "add Y"), mul(f, g, "add Z"), mul(e, h, "add T")
        return mul(e, f, "add X"), mul(g, h, "add Y"), mul(f, g, "add Z"), mul(e, h, "add T")

    for v in ge_double(R, R, R) + ge_add(R, R, R, R, R, R, R, None) + ge_add(R, R, R, R, R, R, R, R):
        need(all(v[i] <= R[i] for i in range(10)), "point op output not reduced")
    # ge_to_pe / ge_from_pa / ge_from_pe
    for v in (carry32(add(R, R)), carry32(sub(R, R, "to_pe ymx")), mul(R, CANON, "to_pe t2d")):
        need(all(v[i] <= R[i] for i in range(10)), "ge_to_pe output not reduced")
    carry32(sub(R, R, "from_pa x"))
    # ge_calc_x
    u = carry32(sub(sqr(FROM_WORDS, "calc y^2"), ONE, "calc u"))
    v = add(mul(R, CANON, "calc d*y^2"), ONE)
    b = sqr(v, "calc v^2")
    a = mul(mul(u, b, "calc u v^2"), v, "calc u v^3")
    b = mul(a, sqr(b, "calc v^4"), "calc u v^7")
    chain250(b, R)
    X = mul(R, a, "calc x")
    to_words(sub(mul(sqr(X, "calc x^2"), v, "calc v x^2"), u, "calc check"), "calc check to_words")
    to_words(X, "calc x to_words")
    carry32(select(neg(X, "calc neg"), X))
    # table generation kernel and the public_fast tail
    carry32(add(CANON, CANON))
    carry32(sub(CANON, CANON, "table B ymx"))
    to_words(add(R, R), "table row to_words")
    to_words(sub(R, R, "table row ymx"), "table row to_words")
    num, den = add(R, R), carry32(sub(R, R, "fast den"))
    chain250(den, R)
    to_words(mul(num, R, "fast u"), "fast to_words")
    print("edwards double / add / decompress / table build / encodings: ok")

    # ---- verify_fast.cuh / blinding (lanes.cuh): rows negated on the fly, the on-curve check, the neutral-element test ----
    t2d_neg = select(neg(R, "pe_cond_neg t2d"), R)           # beta 2 where the row was negated
    for v in ge_add(R, R, R, R, R, R, t2d_neg, R):           # ge_add_pe with a conditionally negated row
        need(all(v[i] <= R[i] for i in range(10)), "add with a negated row: output not reduced")

    def ge_add_pe_row(X, Y, Z, T, ypx, ymx, t2d, z2):        # verify_fast.cuh: the streamed addition's operand order
        a = mul(sub(Y, X, "row add Y-X"), ymx, "row add a")
        b = mul(add(Y, X), ypx, "row add b")
        e, h = sub(b, a, "row add e"), add(b, a)
        c, d = mul(T, t2d, "row add c"), mul(Z, z2, "row add d")
        f, g = sub(d, c, "row add f"), add(d, c)
        return mul(e, f, "row add X"), mul(e, h, "row add T"), mul(g, f, "row add Z"), mul(g, h, "row add Y")

    def ge_add_pa_lds(X, Y, Z, T, ypx, ymx, t2d):            # ... and the streamed affine addition from the LDS table
        a = mul(sub(Y, X, "lds add Y-X"), ymx, "lds add a")
        b = mul(add(Y, X), ypx, "lds add b")
        e, h = sub(b, a, "lds add e"), add(b, a)
        c, d = mul(T, t2d, "lds add c"), add(Z, Z)
        f, g = sub(d, c, "lds add f"), add(d, c)
        return mul(f, e, "lds add X"), mul(e, h, "lds add T"), mul(f, g, "lds add Z"), mul(g, h, "lds add Y")

    for v in ge_add_pe_row(R, R, R, R, R, R, t2d_neg, R) + ge_add_pa_lds(R, R, R, R, CANON, CANON, CANON):
        need(all(v[i] <= R[i] for i in range(10)), "streamed addition: output not reduced")
    # packed table rows (fe_pack_words): what ge_store_pe_row packs -- fe_carry32 outputs and one product -- stays below
    # 2^256 as a positional sum, and what fe_from_words hands back is a legal second operand again
    POS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
    for v, what in ((carry32(add(R, R)), "row Y+X"), (carry32(sub(R, R, "row Y-X")), "row Y-X"), (mul(R, CANON, "row 2dT"), "row 2dT"),
                    (carry32(add(R, R)), "row 2Z")):
        need(sum(x << p for x, p in zip(v, POS)) < 1 << 256, f"packed {what} does not fit 256 bits")
    for v in ge_add_pe_row(R, R, R, R, FROM_WORDS, FROM_WORDS, select(neg(FROM_WORDS, "row neg"), FROM_WORDS), FROM_WORDS):
        need(all(v[i] <= R[i] for i in range(10)), "addition of an unpacked row: output not reduced")
    mul(t2d_neg, CANON, "from_pe T of a negated row")        # ge_from_pe: t2d is the FIRST operand (beta <= 5)
    to_words(add(mul(sqr(R, "check x^2"), add(R, ONE), "check v x^2"), R), "calc check c + u")      # ge_calc_x_checked
    to_words(sub(R, R, "neutral Y - Z"), "neutral test to_words")
    carry32(neg(R, "negate X / T of R and Q"))
    # ge_from_pa with the blinding context's random Z: all four coordinates times zr (reduced from words), Z = carry32(2 zr)
    for v in (mul(carry32(sub(R, R, "blind x")), FROM_WORDS, "blind X*zr"), mul(R, FROM_WORDS, "blind T*zr"),
              carry32(add(FROM_WORDS, FROM_WORDS))):
        need(all(v[i] <= R[i] for i in range(10)), "blinded start not reduced")
    # ---- ge25519.cuh signed comb (ge_base_mult): rows leave LDS negated when their column's top digit is -1 ----
    for v in ge_add(R, R, R, R, R, R, t2d_neg, None):        # ge_add_pa with a conditionally negated affine row
        need(all(v[i] <= R[i] for i in range(10)), "signed comb: add with a negated affine row: output not reduced")
    mul(t2d_neg, CANON, "signed comb: ge_from_pa T of a negated first row")
    carry32(neg(CANON, "signed comb table generation: -B's 2dxy"))
    print("lattice verification walk, signed comb and blinded base walk: ok")
    # ---- verify_ctx_zip215.cuh: the coset comparison behind the context walks (X, Y, Z reduced: the walk's last products) ----
    def coset_denominators(X, Y, Z):
        zz = sqr(Z, "coset Z^2")
        kxy = mul(mul(X, Y, "coset XY"), CANON, "coset kXY")
        return add(zz, kxy), sub(zz, kxy, "coset dm")

    dp, dm = coset_denominators(R, R, R)
    W = mul(mul(dm, dp, "coset prep dm*dp"), R, "coset prep W")                    # coset_prep_element
    need(all(W[i] <= R[i] for i in range(10)), "coset prep: W not reduced")
    w_inv = R                                                                       # the shared inversion's output: a product, or zero
    to_words(w_inv, "coset w_inv to_words")
    z_inv = mul(mul(dm, dp, "coset dm*dp"), w_inv, "coset 1/Z")                     # coset_contains_r
    t = mul(mul(w_inv, R, "coset w_inv*Z"), R, "coset w_inv*Z^2")
    zdp, zdm = mul(dm, t, "coset Z/dp"), mul(dp, t, "coset Z/dm")
    x, y = mul(R, z_inv, "coset x"), mul(R, z_inv, "coset y")
    for v in (x, y, mul(y, CANON, "coset i*y"), mul(x, CANON, "coset i*x")):
        to_words(v, "coset candidate to_words")
    a, b = mul(R, CANON, "coset X*y8"), mul(R, CANON, "coset Y*x8")
    for num, den in ((add(a, b), zdp), (add(a, b), zdm), (sub(a, b, "coset a-b"), zdm), (sub(a, b, "coset c-e"), zdp)):
        to_words(mul(num, den, "coset candidate of the order-8 family"), "coset candidate to_words")
    # zip215_ctx_key_ok: the curve equation on row 1 of a context (its fields read by fe_from_words), and its y against the key's
    x2, y2 = sub(FROM_WORDS, FROM_WORDS, "key_ok 2x"), add(FROM_WORDS, FROM_WORDS)
    xx, yy = sqr(x2, "key_ok (2x)^2"), sqr(y2, "key_ok (2y)^2")
    lhs = chained_small_mul(sub(yy, xx, "key_ok yy-xx"), 4, [0] * 10, "key_ok 4(yy-xx)")
    rhs = add(mul(mul(xx, yy, "key_ok xx*yy"), CANON, "key_ok d*xx*yy"), [16] + [0] * 9)
    to_words(sub(lhs, rhs, "key_ok lhs-rhs"), "key_ok curve equation to_words")
    to_words(sub(y2, carry32(add(FROM_WORDS, FROM_WORDS), "key_ok 2 y_key"), "key_ok y"), "key_ok y to_words")
    print("ZIP-215 coset comparison against contexts (prep, finish, rule 2 per context): ok")
    # ---- ed_keys.cuh: the walk [L]A from the decoder's (x, y) -- x a fe_carry32 output, y fresh from words -- and the conversion ----
    x, y = carry32(select(neg(R, "key x neg"), R)), FROM_WORDS
    A_ypx, A_ymx = carry32(add(y, x)), carry32(sub(y, x, "key Y-X"))
    A_t2d = mul(mul(x, y, "key xy"), CANON, "key 2dxy")
    for v in (A_ypx, A_ymx, A_t2d):
        need(all(v[i] <= R[i] for i in range(10)), "key walk: A's precomputed form not reduced")
    S = ge_double(x, y, ONE)                                 # the first doubling starts from (x, y, 1) ...
    for v in S:
        need(all(v[i] <= R[i] for i in range(10)), "key walk: first doubling not reduced")
    for v in ge_add(R, R, R, R, select(A_ypx, A_ymx), select(A_ypx, A_ymx), select(neg(A_t2d, "key -2dxy"), A_t2d), None):
        need(all(v[i] <= R[i] for i in range(10)), "key walk: addition of +-A not reduced")     # ... every later step from reduced S
    to_words(sub(R, R, "key neutral Y - Z"), "key neutral test to_words")
    to_words(x, "key x to_words")
    num, den = carry32(add(ONE, y)), carry32(sub(ONE, y, "key 1 - y"))
    need(all(num[i] <= R[i] and den[i] <= R[i] for i in range(10)), "key conversion: 1 + y / 1 - y not reduced")
    to_words(mul(num, R, "key u"), "key u to_words")
    print("key classification walk [L]A and conversion to X25519: ok")
    # ---- ristretto255.cuh: SQRT_RATIO_M1, DECODE, ENCODE and the Elligator MAP (RFC 9496) ----
    def reduced(v, what):
        need(all(v[i] <= R[i] for i in range(10)), f"{what} not reduced")
        return v

    def rist_cneg(a, what):                                  # fe_neg, fe_select, fe_carry32
        return reduced(carry32(select(neg(a, f"{what} neg"), a), what), what)

    def rist_abs(a, what):
        to_words(a, f"{what} parity")
        return rist_cneg(a, what)

    def rist_sqrt_ratio(u, v, unit_u, what):                 # u, v reduced
        b = sqr(v, f"{what} v^2")
        a = mul(b, v, f"{what} v^3")
        if not unit_u:
            a = mul(a, u, f"{what} u v^3")
        b = mul(a, sqr(b, f"{what} v^4"), f"{what} u v^7")
        chain250(b, R)
        r = mul(R, a, f"{what} r")
        check = mul(sqr(r, f"{what} r^2"), v, f"{what} check")
        ui = CANON if unit_u else mul(u, CANON, f"{what} u sqrt(-1)")
        to_words(sub(check, u, f"{what} check - u"), f"{what} correct")
        to_words(add(check, u), f"{what} flipped")
        to_words(add(check, ui), f"{what} flipped_i")
        return rist_abs(select(mul(r, CANON, f"{what} r sqrt(-1)"), r), f"{what} |r|")

    def rist_decode():
        s = FROM_WORDS
        ss = sqr(s, "decode s^2")
        u1 = reduced(carry32(sub(ONE, ss, "decode 1 - ss")), "decode u1")
        u2 = add(ss, ONE)
        u2s = sqr(u2, "decode u2^2")
        t = carry32(add(mul(sqr(u1, "decode u1^2"), CANON, "decode d u1^2"), u2s))
        v = reduced(carry32(neg(t, "decode -t")), "decode v")
        inv = rist_sqrt_ratio(ONE, mul(v, u2s, "decode v u2^2"), True, "decode sqrt")
        dx = mul(inv, u2, "decode den_x")
        dy = mul(mul(inv, dx, "decode inv den_x"), v, "decode den_y")
        X = rist_abs(mul(add(s, s), dx, "decode 2 s den_x"), "decode x")
        Y = mul(u1, dy, "decode y")
        to_words(mul(X, Y, "decode t"), "decode t parity")
        to_words(Y, "decode y == 0")
        return rist_cneg(X, "decode -x"), reduced(Y, "decode y")

    def rist_encode(X, Y, Z, T, has_t):
        if not has_t:
            X, Y, T, Z = mul(X, Z, "encode XZ"), mul(Y, Z, "encode YZ"), mul(X, Y, "encode XY"), sqr(Z, "encode Z^2")
        u1 = mul(sub(Z, Y, "encode Z - Y"), add(Z, Y), "encode u1")
        u2 = mul(X, Y, "encode u2")
        inv = rist_sqrt_ratio(ONE, mul(u1, sqr(u2, "encode u2^2"), "encode u1 u2^2"), True, "encode sqrt")
        d1, d2 = mul(inv, u1, "encode den1"), mul(inv, u2, "encode den2")
        zi = mul(mul(d1, d2, "encode den1 den2"), T, "encode z_inv")
        to_words(mul(T, zi, "encode t z_inv"), "encode rotate")
        x = select(mul(Y, CANON, "encode iy"), X)
        y = select(mul(X, CANON, "encode ix"), Y)
        di = select(mul(d1, CANON, "encode enchanted"), d2)
        to_words(mul(x, zi, "encode x z_inv"), "encode neg y")
        y = rist_cneg(y, "encode -y")
        to_words(mul(sub(Z, y, "encode Z - y"), di, "encode s"), "encode s to_words")

    def rist_map(t):
        r = mul(sqr(t, "map t^2"), CANON, "map r")
        u = mul(add(r, ONE), CANON, "map u")
        a = neg(add(mul(r, CANON, "map r d"), ONE), "map -1 - r d")
        v = mul(a, add(r, CANON), "map v")
        s = rist_sqrt_ratio(u, v, False, "map sqrt")
        sp = rist_cneg(mul(s, t, "map s t"), "map s'")
        to_words(mul(s, t, "map s t"), "map s t parity")
        s = select(s, sp)
        c = select(neg(ONE, "map -1"), r)
        n = mul(mul(sub(r, ONE, "map r - 1"), c, "map c (r - 1)"), CANON, "map c (r - 1)(d - 1)^2")
        n = sub(n, v, "map N")
        w0 = mul(add(s, s), v, "map w0")
        w1 = mul(n, CANON, "map w1")
        w3 = sqr(s, "map s^2")
        w2 = sub(ONE, w3, "map w2")
        w3 = add(w3, ONE)
        return (reduced(mul(w0, w3, "map X"), "map X"), reduced(mul(w2, w1, "map Y"), "map Y"), reduced(mul(w1, w3, "map Z"), "map Z"),
                reduced(mul(w2, w0, "map T"), "map T"))

    x, y = rist_decode()
    for v in ge_add(x, y, ONE, mul(x, y, "rist add T"), carry32(add(y, x)), carry32(sub(y, x, "rist add Y-X")),
                    mul(mul(x, y, "rist add xy"), CANON, "rist add 2dxy"), None):
        reduced(v, "ristretto255 PointAdd")
    rist_encode(R, R, R, R, True)                            # PointAdd, FromHash: the addition's own T
    rist_encode(R, R, R, R, False)                           # ScalarMult, ScalarMultBase: re-formed from the walk's (X, Y, Z)
    P1 = rist_map(FROM_WORDS)
    for v in ge_add(*P1, carry32(add(P1[1], P1[0])), carry32(sub(P1[1], P1[0], "rist pe ymx")), mul(P1[3], CANON, "rist pe t2d"),
                    carry32(add(P1[2], P1[2]))):
        reduced(v, "ristretto255 FromHash addition")
    print("ristretto255 square-root step, decode, encode (with T and re-formed), Elligator map: ok")
    # ---- h2c25519.cuh: the 48-byte reduction and the Elligator 2 map to the Edwards curve (RFC 9380 appendix G.2) ----
    def h2c_fe_from_be48():
        hi = [M26, M25, M26, M25, M26] + [0] * 5              # 128 bits through fe_from_words: five limbs (bit 255 of `hi` is clear)
        a = [FROM_WORDS[i] + 38 * hi[i] for i in range(10)]
        need(all(x <= U32 for x in a), "be48: lo + 38 hi overflows 32 bits")
        need(beta(a) <= CONTRACT["carry32"], f"be48: beta {beta(a):.2f} outside fe_carry32's contract")
        return reduced(carry32(a, "be48 carry"), "be48")

    def h2c_eq(a, b, what):                                  # fe_sub, then rist_is_zero's fe_to_words
        to_words(sub(a, b, f"{what} sub"), f"{what} to_words")

    def h2c_map(u):
        J = [486662] + [0] * 9
        tv1 = reduced(carry32(add(sqr(u, "h2c u^2"), sqr(u, "h2c u^2")), "h2c tv1"), "h2c tv1")
        xd = add(tv1, ONE)
        tv2 = sqr(xd, "h2c xd^2")
        gxd = mul(tv2, xd, "h2c gxd")
        gx1 = mul(mul(tv1, J, "h2c J tv1"), CANON, "h2c x1n J tv1")
        gx1 = mul(add(gx1, tv2), CANON, "h2c gx1")
        tv3 = sqr(gxd, "h2c gxd^2")
        tv2 = sqr(tv3, "h2c gxd^4")
        tv3 = mul(mul(tv3, gxd, "h2c gxd^3"), gx1, "h2c gx1 gxd^3")
        tv2 = mul(tv2, tv3, "h2c gx1 gxd^7")
        chain250(tv2, R)
        y11 = mul(R, tv3, "h2c y11")
        y12 = mul(y11, CANON, "h2c y12")
        h2c_eq(mul(sqr(y11, "h2c y11^2"), gxd, "h2c y11^2 gxd"), gx1, "h2c e1")
        y1 = select(y11, y12)
        x2n = mul(tv1, CANON, "h2c x2n")
        y21 = mul(mul(y11, u, "h2c y11 u"), CANON, "h2c y21")
        y22 = mul(y21, CANON, "h2c y22")
        gx2 = mul(gx1, tv1, "h2c gx2")
        h2c_eq(mul(sqr(y21, "h2c y21^2"), gxd, "h2c y21^2 gxd"), gx2, "h2c e2")
        y2 = select(y21, y22)
        h2c_eq(mul(sqr(y1, "h2c y1^2"), gxd, "h2c y1^2 gxd"), gx1, "h2c e3")
        xn, y = select(CANON, x2n), select(y1, y2)
        y = rist_abs(y, "h2c sgn0 fix-up")                   # fe_to_words for the parity, then rist_cneg
        en, ed = mul(xn, CANON, "h2c xn c1"), mul(xd, y, "h2c xd y")
        yn = reduced(carry32(sub(xn, xd, "h2c xn - xd")), "h2c yn")
        yd = reduced(carry32(add(xn, xd)), "h2c yd")
        to_words(mul(ed, yd, "h2c denominators"), "h2c exceptional")
        en, ed, yn, yd = select(en, [0] * 10), select(ed, ONE), select(yn, ONE), select(yd, ONE)
        return (reduced(mul(en, yd, "h2c X"), "h2c X"), reduced(mul(yn, ed, "h2c Y"), "h2c Y"), reduced(mul(ed, yd, "h2c Z"), "h2c Z"),
                reduced(mul(en, yn, "h2c T"), "h2c T"))

    Q = h2c_map(select(h2c_fe_from_be48(), FROM_WORDS))      # u from 48 expander bytes, or MapToCurve's 32 with bit 255 masked
    for v in ge_add(*Q, carry32(add(Q[1], Q[0])), carry32(sub(Q[1], Q[0], "h2c pe ymx")), mul(Q[3], CANON, "h2c pe t2d"),
                    carry32(add(Q[2], Q[2]))):
        reduced(v, "HashToCurve addition")
    for v in ge_double(R, R, R):
        reduced(v, "HashToCurve doubling")
    to_words(mul(R, R, "h2c affine"), "h2c encode to_words")
    print("hash to curve: 48-byte reduction (beta 39 into one carry pass), Elligator 2 map, addition, doublings, encoding: ok")
    quad_section(R)
    print("quad25519 ladder step, addition, doubling, batch-inversion exchange: ok")
    small = coop_section(R)
    print(f"coop25519 carry_small output class: beta <= {beta(small):.6f} (limb0 <= 2^26 + {small[0] - (1 << 26)})")
    print("coop25519 products, carries, ladder, two-wave ladder, mont_double, edwards add / double: ok")
    print("all bounds hold")


if __name__ == "__main__":
    main()
