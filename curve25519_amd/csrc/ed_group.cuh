// curve25519_amd/csrc/ed_group.cuh -- what ONE lane does for the group calls (include/curve25519_amd.h states their rules):
//   ed25519_ScalarMult[_noclamp]_*       [e]P for a variable point P under a SECRET scalar e
//   ed25519_ScalarMultBase[_noclamp]_*   [e]B over the wide comb
//   ed25519_PointAdd_* / PointSub_*      P + Q, P - Q
// engine_group.hip wraps these in its kernels; tests/host_emul/group_ops.cpp drives the same functions on the CPU.
//
// The new work is a variable-base walk under a secret scalar: the library's other walks run over tables built for a fixed point
// (combs, peer contexts), under a public per-element scalar (verification) or under a public constant ([L]A).  Here the table is
// built per element and nothing may depend on the scalar but data: no branch condition, no load or store address.
//   * Recoding.  e < 2^255 is written in N signed W-bit digits d_i in [-R, R - 1], R = 2^(W-1), by ONE addition: with
//     C = sum_i R * 2^(W i) the W-bit fields of e + C are d_i + R, since sum_i (f_i - R) 2^(W i) = e + C - C.  The carries of a
//     digit-by-digit recoding are the carries of that addition, so no digit needs one of its own.  e + C must fit N fields:
//     N = 129 / 86 / 65 for W = 2 / 3 / 4 (C is 2/3, 4/7, 8/15 of 2^(W N); the obvious 128 and 64 fields are one short: the sum
//     overflows from 2/3 of 2^255 at W = 2, 2^254 + 2^253 for one, and from 14/15 of 2^255 at W = 4).
//   * Table.  Rows 1P .. RP in ge_pe form, in registers (2 / 4 / 8 rows of 40 limbs), built by R - 1 complete additions of P.
//   * Select.  |d| is compared with every row number and the rows are combined under the resulting all-ones / zero masks; |d| = 0
//     selects the neutral row (1, 1, 0, 2).  A negative digit swaps Y+X and Y-X and negates 2dT, again by mask.
//   * Walk.  From the neutral element, per digit: W - 1 doublings that do not form T, one that does, one addition that does not
//     (a doubling does not read T, and neither does the encoding).  The digits leave the recoded scalar from the top by a shift of
//     the whole register array, so the loop stays rolled without a register index.
// The additions are the complete ones of ge25519.cuh (a = -1, d not a square): points of small or mixed order, the neutral element
// and P + P need no case of their own.  Everything on the scalar's path is written with masks: a ?: on a secret is a branch at -O1
// in the taint build (tests/host_emul/taint_group_ops.cpp).  Points are public; their decoding may branch and does not.
#pragma once
#include "lanes.cuh"
#include "verify_fast.cuh"

namespace c25519 {

template <int W> struct GroupWindow {
    static_assert(W >= 2 && W <= 4, "window widths 2, 3 and 4");
    static constexpr int ROWS = 1 << (W - 1);
    static constexpr int DIGITS = W == 2 ? 129 : W == 3 ? 86 : 65;
    static constexpr int BITS = W * DIGITS;                  // 258, 258, 260
    static constexpr int WORDS = 9;
    static constexpr int SHIFT = 32 * WORDS - BITS;          // the top digit sits in the top W bits of word 8
};

// C = sum_i R * 2^(W i): bit W i + W - 1 for every digit i
template <int W> struct GroupOffset { u32 w[GroupWindow<W>::WORDS]; };
template <int W>
C25519_DEV constexpr GroupOffset<W> group_offset()
{
    GroupOffset<W> c{};
    for (int i = 0; i < GroupWindow<W>::DIGITS; i++) {
        const int bit = W * i + W - 1;
        c.w[bit >> 5] |= 1u << (bit & 31);
    }
    return c;
}

// e as the calls read a 32-byte scalar: clamp = all-ones: clamped on this copy; zero: the low 255 bits
C25519_DEV void group_scalar(u32 (&e)[8], const u32 (&s)[8], u32 clamp)
{
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = s[i];
    e[0] &= ~(7u & clamp);
    e[7] = (e[7] & 0x7fffffffu) | (0x40000000u & clamp);
}

// t = (e + C) << SHIFT, e < 2^255
template <int W>
C25519_DEV void group_recode(u32 (&t)[9], const u32 (&e)[8])
{
    constexpr int S = GroupWindow<W>::SHIFT;
    constexpr GroupOffset<W> C = group_offset<W>();
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (u64)e[i] + C.w[i];
        t[i] = (u32)c;
        c >>= 32;
    }
    t[8] = (u32)c + C.w[8];
#pragma unroll
    for (int i = 8; i > 0; i--) t[i] = (t[i] << S) | (t[i - 1] >> (32 - S));
    t[0] <<= S;
}

// the next digit from the top, as its field d + R in [0, 2^W)
template <int W>
C25519_DEV u32 group_next_field(u32 (&t)[9])
{
    const u32 f = t[8] >> (32 - W);
#pragma unroll
    for (int i = 8; i > 0; i--) t[i] = (t[i] << W) | (t[i - 1] >> (32 - W));
    t[0] <<= W;
    return f;
}

// all-ones iff a == b (a, b < 2^31)
C25519_DEV u32 group_eq_mask(u32 a, u32 b) { return 0u - (((a ^ b) - 1u) >> 31); }

// q = d * P for the field f = d + R: rows[j] = (j + 1) P
template <int W>
C25519_DEV void group_select(ge_pe& q, const ge_pe (&rows)[GroupWindow<W>::ROWS], u32 f)
{
    constexpr u32 R = GroupWindow<W>::ROWS;
    const u32 neg = ((f >> (W - 1)) & 1u) - 1u;              // all-ones: f < R, a negative digit
    const u32 mag = ((f - R) ^ neg) - neg;                   // |d| in [0, R]
    const u32 zero = group_eq_mask(mag, 0);
    fe ypx, ymx, t2d, n;
    fe_set_u32(ypx, 1u & zero);
    fe_set_u32(ymx, 1u & zero);
    fe_set_u32(t2d, 0);
    fe_set_u32(q.z2, 2u & zero);
#pragma unroll
    for (u32 j = 0; j < R; j++) {
        const u32 m = group_eq_mask(mag, j + 1);
#pragma unroll
        for (int i = 0; i < 10; i++) {
            ypx.v[i] |= rows[j].ypx.v[i] & m;
            ymx.v[i] |= rows[j].ymx.v[i] & m;
            t2d.v[i] |= rows[j].t2d.v[i] & m;
            q.z2.v[i] |= rows[j].z2.v[i] & m;
        }
    }
    fe_select(q.ypx, neg, ymx, ypx);
    fe_select(q.ymx, neg, ypx, ymx);
    fe_neg(n, t2d);                                          // 2p - 2dT: beta 2, fine as the second factor of a product
    fe_select(q.t2d, neg, n, t2d);
}

// S = [e](x, y), e < 2^255, for affine x, y with reduced limbs; T of the result is not formed
template <int W>
C25519_DEV void ed_group_walk(ge_ext& S, const fe& x, const fe& y, const u32 (&e)[8])
{
    constexpr int R = GroupWindow<W>::ROWS;
    ge_pe rows[R];
    {
        ge_ext Q;
        Q.X = x;
        Q.Y = y;
        fe_set_u32(Q.Z, 1);
        fe_mul(Q.T, x, y);
        ge_to_pe(rows[0], Q);
#pragma unroll
        for (int j = 1; j < R; j++) {
            ge_add_pe<true>(Q, Q, rows[0]);
            ge_to_pe(rows[j], Q);
        }
    }
    u32 t[9];
    group_recode<W>(t, e);
    fe_set_u32(S.X, 0);
    fe_set_u32(S.Y, 1);
    fe_set_u32(S.Z, 1);
    fe_set_u32(S.T, 0);
#pragma unroll 1
    for (int i = 0; i < GroupWindow<W>::DIGITS; i++) {
#pragma unroll 1
        for (int d = 0; d < W - 1; d++) ge_double<false>(S);
        ge_double<true>(S);
        ge_pe q;
        group_select<W>(q, rows, group_next_field<W>(t));
        ge_add_pe<false>(S, S, q);
    }
}

// ed25519_ScalarMult[_noclamp] for one element: S = [e]P projective, returns all-ones iff the point bytes decode (a point that
// does not decode walks too: the output is masked)
template <int W>
C25519_DEV u32 ed_group_scalarmult_lane(ge_ext& S, const u32 (&sw)[8], const u32 (&pw)[8], u32 clamp)
{
    fe X, Y;
    const u32 ok = ed_zip215_decode(X, Y, pw, 0u);
    u32 e[8];
    group_scalar(e, sw, clamp);
    ed_group_walk<W>(S, X, Y, e);
    return ok;
}

// ed25519_ScalarMultBase[_noclamp] for one element: S = [e]B over the wide comb (B has order L: the comb's own e + L for an even e);
// cols: this lane's parked columns, `stride` elements apart
template <typename ColT>
C25519_DEV void ed_group_base_lane(ge_ext& S, const u32 (&sw)[8], u32 clamp, const u32* __restrict__ g_wide, ColT* cols, int stride)
{
    u32 e[8];
    group_scalar(e, sw, clamp);
    wb_columns(cols, stride, e);
    ge_base_mult_wide(S, g_wide, cols, stride);
}

// ed25519_PointAdd / PointSub for one element: S = P + Q (negate = zero) or P - Q (all-ones) projective, returns all-ones iff both
// decode.  -Q is (-x, y): the decoder hands it back negated.
C25519_DEV u32 ed_group_add_lane(ge_ext& S, const u32 (&pw)[8], const u32 (&qw)[8], u32 negate)
{
    fe X, Y, t;
    u32 ok = ed_zip215_decode(X, Y, pw, 0u);
    S.X = X;
    S.Y = Y;
    fe_set_u32(S.Z, 1);
    fe_mul(S.T, X, Y);
    ok &= ed_zip215_decode(X, Y, qw, negate);
    ge_pa A;
    fe_add(t, Y, X);  fe_carry32(A.ypx, t);
    fe_sub(t, Y, X);  fe_carry32(A.ymx, t);
    fe_mul(t, X, Y);
    fe_mul(A.t2d, t, fe_const(K_2D));
    ge_add_pa<false>(S, A);
    return ok;
}

// the shared inversion's output for ScalarMult, PointAdd and PointSub: out = enc(X / Z, Y / Z) where the element's ok word is set
// (y < p, bit 255 the parity of x; the neutral element is 01 00 .. 00), 32 zero bytes where it is not
struct FinishGroupPoint {
    const u32 *X, *Y, *ok; void* out; size_t n;
    C25519_DEV bool skip() const { return false; }
    C25519_DEV void emit(size_t e, const fe& zinv) const
    {
        fe t;
        u32 xw[8], yw[8], enc[8];
        soa_load_fe(t, X, n, e);  fe_mul(t, t, zinv);  fe_to_words(xw, t);
        soa_load_fe(t, Y, n, e);  fe_mul(t, t, zinv);  fe_to_words(yw, t);
        ge_pack(enc, xw, yw);
        const u32 keep = ok[e];
#pragma unroll
        for (int i = 0; i < 8; i++) enc[i] &= keep;
        store32(out, e, enc);
    }
};

}  // namespace c25519
