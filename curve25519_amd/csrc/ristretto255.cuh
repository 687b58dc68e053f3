// curve25519_amd/csrc/ristretto255.cuh -- what ONE lane does for the ristretto255 calls (RFC 9496; include/curve25519_amd.h states
// their rules):
//   ristretto255_IsValidPoint_*       DECODE succeeds
//   ristretto255_FromHash_*           ENCODE(MAP(low half) + MAP(high half))
//   ristretto255_ScalarMult_*         ENCODE([e] DECODE(point)) under a SECRET scalar e: ed_group.cuh's walk between the two
//   ristretto255_ScalarMultBase_*     ENCODE([e]B) over the wide comb
//   ristretto255_PointAdd_* / Sub_*   ENCODE(DECODE(p) +- DECODE(q))
// engine_ristretto.hip wraps these in its kernels; tests/host_emul/ristretto.cpp drives the same functions on the CPU.
//
// ristretto255 is the prime-order quotient of the Edwards group by its 8-torsion (over a 4-torsion it shares with the Jacobi
// quartic): an element is a coset of four points, DECODE hands back one representative as an affine (x, y) -- what ed_group_walk
// and the complete additions of ge25519.cuh take -- and ENCODE gives the same 32 bytes for all four.  Each of DECODE, ENCODE and MAP
// is built on SQRT_RATIO_M1, one x^((p-5)/8) chain (fe_pow2523: 254 squarings and 11 products with the products around it).
//   * The inverse square root of ENCODE is per element and is NOT shared: Montgomery's trick shares an inversion because
//     1 / (a b) splits into 1 / a and 1 / b by products; 1 / sqrt(a b) does not say which of a, b was a square, and ENCODE's
//     choices (rotate, the two negations) hang on exactly that.  So ENCODE runs in the lane, leases no scratch and launches no
//     k_batch_invert; a call is ONE kernel.
//   * ENCODE reads T.  The walk's last addition and the comb's do not form it (ed_group.cuh, ge25519.cuh: a doubling or an affine
//     conversion never read T), and they stay as they are: rist_encode<false> RE-FORMS the point as (X Z, Y Z, Z^2, X Y), the same
//     projective point with T' = X' Y' / Z', for three products and a squaring.  Where the addition is this header's own (PointAdd,
//     FromHash) it is instantiated with T and rist_encode<true> takes the point as it is.
//   * Everything is written with masks (all-ones / zero words): comparisons are made on canonical words (fe_to_words), selections
//     by fe_select, negations by selecting between a value and its negative.  No ?: and no branch anywhere: the scalar reaches
//     ENCODE through [e]P, and the 64 hash bytes are secret from the first instruction of MAP (tests/host_emul/taint_ristretto.cpp).
//     Point encodings are public, and DECODE does not branch on them either: a row that does not decode walks like any other and its
//     output is masked.
// Limb bounds (fe25519.cuh's contract; tools/fe_bounds.py replays decode, encode and map): every value named below is reduced unless
// a comment gives its beta.
#pragma once
#include "lanes.cuh"
#include "verify_fast.cuh"
#include "strict25519.cuh"
#include "ed_group.cuh"

namespace c25519 {

// all-ones iff a == 0 mod p
C25519_DEV u32 rist_is_zero(const fe& a)
{
    u32 w[8], nz = 0;
    fe_to_words(w, a);
#pragma unroll
    for (int i = 0; i < 8; i++) nz |= w[i];
    return ((nz | (0u - nz)) >> 31) - 1u;
}

// all-ones iff the canonical value of a is odd ("negative", RFC 9496 section 4.1)
C25519_DEV u32 rist_is_negative(const fe& a)
{
    u32 w[8];
    fe_to_words(w, a);
    return 0u - (w[0] & 1u);
}

// r = -a where mask is all-ones, a where it is zero; a reduced, r reduced
C25519_DEV void rist_cneg(fe& r, const fe& a, u32 mask)
{
    fe n;
    fe_neg(n, a);                                            // beta 2
    fe_select(n, mask, n, a);
    fe_carry32(r, n);
}

// r = |a|: the even one of a, -a
C25519_DEV void rist_abs(fe& r, const fe& a) { rist_cneg(r, a, rist_is_negative(a)); }

// SQRT_RATIO_M1(u, v), RFC 9496 section 4.2: r = the non-negative square root of u / v where there is one (returns all-ones; also
// for u = 0), of sqrt(-1) u / v where there is none (returns zero); v = 0 gives r = 0 and zero.  u, v reduced.  UNIT_U: u is 1
// (DECODE and ENCODE take an INVERSE square root) and is read by the comparisons alone: two products fewer.
//   r = (u v^3) (u v^7)^((p-5)/8); check = v r^2 is u, -u, or +-u sqrt(-1)
template <bool UNIT_U>
C25519_DEV u32 rist_sqrt_ratio(fe& r, const fe& u, const fe& v)
{
    fe a, b, check, t;
    fe_sqr(b, v);                                            // v^2
    fe_mul(a, b, v);                                         // v^3
    if (!UNIT_U) fe_mul(a, a, u);                            // u v^3
    fe_sqr(b, b);                                            // v^4
    fe_mul(b, a, b);                                         // u v^7
    fe_pow2523(b, b);
    fe_mul(r, b, a);
    fe_sqr(check, r);
    fe_mul(check, check, v);
    fe ui;
    if (UNIT_U) ui = fe_const(K_SQRTM1);
    else fe_mul(ui, u, fe_const(K_SQRTM1));
    fe_sub(t, check, u);                                     // beta 3
    const u32 correct = rist_is_zero(t);
    fe_add(t, check, u);                                     // beta 2
    const u32 flipped = rist_is_zero(t);
    fe_add(t, check, ui);                                    // beta 2
    const u32 flipped_i = rist_is_zero(t);
    fe_mul(t, r, fe_const(K_SQRTM1));
    fe_select(r, flipped | flipped_i, t, r);
    rist_abs(r, r);
    return correct | flipped;
}

// DECODE, RFC 9496 section 4.3.1: (X, Y) affine and reduced, -X where `negate` is all-ones (PointSub's second operand); returns
// all-ones iff the 32 bytes decode.  One inverse square root.
C25519_DEV u32 rist_decode(fe& X, fe& Y, const u32 (&w)[8], u32 negate)
{
    u32 ok = strict_less(w, K_P) & ((w[0] & 1u) - 1u);       // s < p (so bit 255 is clear) and s even
    fe s, ss, u1, u2, u2s, v, vu, inv, one, t;
    fe_set_u32(one, 1);
    fe_from_words(s, w);
    fe_sqr(ss, s);
    fe_sub(t, one, ss);  fe_carry32(u1, t);                  // u1 = 1 - s^2
    u2 = ss;
    u2.v[0] += 1;                                            // u2 = 1 + s^2
    fe_sqr(u2s, u2);
    fe_sqr(t, u1);
    fe_mul(t, t, fe_const(K_D));
    fe_add(t, t, u2s);                                       // beta 2
    fe_carry32(t, t);
    fe_neg(t, t);                                            // beta 2
    fe_carry32(v, t);                                        // v = -(d u1^2) - u2^2
    fe_mul(vu, v, u2s);
    ok &= rist_sqrt_ratio<true>(inv, one, vu);
    fe dx, dy;
    fe_mul(dx, inv, u2);                                     // den_x
    fe_mul(dy, inv, dx);
    fe_mul(dy, dy, v);                                       // den_y
    fe_add(t, s, s);                                         // beta 2
    fe_mul(t, t, dx);
    rist_abs(X, t);                                          // x = |2 s den_x|
    fe_mul(Y, u1, dy);
    fe_mul(t, X, Y);
    ok &= ~rist_is_negative(t) & ~rist_is_zero(Y);
    rist_cneg(X, X, negate);
    return ok;
}

// ENCODE, RFC 9496 section 4.3.2: the 32 bytes of the element S represents, as 8 words.  HAS_T = false: S.T is not read and the
// point is re-formed as (X Z, Y Z, Z^2, X Y) first (the header comment says why).  One inverse square root.
template <bool HAS_T>
C25519_DEV void rist_encode(u32 (&out)[8], const ge_ext& S)
{
    fe X, Y, Z, T;
    if (HAS_T) {
        X = S.X;  Y = S.Y;  Z = S.Z;  T = S.T;
    } else {
        fe_mul(X, S.X, S.Z);
        fe_mul(Y, S.Y, S.Z);
        fe_mul(T, S.X, S.Y);
        fe_sqr(Z, S.Z);
    }
    fe u1, u2, inv, d1, d2, zi, t, a, one;
    fe_set_u32(one, 1);
    fe_add(a, Z, Y);                                         // beta 2
    fe_sub(t, Z, Y);                                         // beta 3
    fe_mul(u1, t, a);                                        // u1 = (Z + Y)(Z - Y)
    fe_mul(u2, X, Y);
    fe_sqr(t, u2);
    fe_mul(t, u1, t);
    (void)rist_sqrt_ratio<true>(inv, one, t);
    fe_mul(d1, inv, u1);
    fe_mul(d2, inv, u2);
    fe_mul(zi, d1, d2);
    fe_mul(zi, zi, T);                                       // z_inv
    fe_mul(t, T, zi);
    const u32 rotate = rist_is_negative(t);
    fe x, y, di;
    fe_mul(t, Y, fe_const(K_SQRTM1));                        // iy0
    fe_select(x, rotate, t, X);
    fe_mul(t, X, fe_const(K_SQRTM1));                        // ix0
    fe_select(y, rotate, t, Y);
    fe_mul(t, d1, fe_const(K_INVSQRT_A_MINUS_D));            // the enchanted denominator
    fe_select(di, rotate, t, d2);
    fe_mul(t, x, zi);
    rist_cneg(y, y, rist_is_negative(t));
    fe_sub(t, Z, y);                                         // beta 3
    fe_mul(t, t, di);
    // |s| on the canonical words: p - s where s is odd (s odd is not 0, so p - s is in [1, p - 1])
    u32 sw[8], nw[8];
    fe_to_words(sw, t);
    const u32 odd = 0u - (sw[0] & 1u);
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 d = (u64)K_P[i] - sw[i] - borrow;
        nw[i] = (u32)d;
        borrow = (d >> 63) & 1u;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = (nw[i] & odd) | (sw[i] & ~odd);
}

// the Elligator MAP, RFC 9496 section 4.3.4, in the RFC's operation order: P = MAP(t) in extended coordinates, t reduced.  One
// square-root chain.
C25519_DEV void rist_map(ge_ext& P, const fe& t)
{
    fe r, u, v, s, c, n, a, b, one;
    fe_set_u32(one, 1);
    fe_sqr(r, t);
    fe_mul(r, r, fe_const(K_SQRTM1));                        // r = sqrt(-1) t^2
    a = r;
    a.v[0] += 1;
    fe_mul(u, a, fe_const(K_ONE_MINUS_D_SQ));                // u = (r + 1)(1 - d^2)
    fe_mul(a, r, fe_const(K_D));
    a.v[0] += 1;
    fe_neg(a, a);                                            // -1 - r d, beta 2
    fe_add(b, r, fe_const(K_D));                             // r + d, beta 2
    fe_mul(v, a, b);
    const u32 was_square = rist_sqrt_ratio<false>(s, u, v);
    fe_mul(a, s, t);
    rist_cneg(a, a, ~rist_is_negative(a));                   // s' = -|s t|
    fe_select(s, was_square, s, a);
    fe_neg(a, one);                                          // -1, beta 2
    fe_select(c, was_square, a, r);                          // beta 2
    fe_sub(a, r, one);                                       // r - 1, beta 3
    fe_mul(n, a, c);
    fe_mul(n, n, fe_const(K_D_MINUS_ONE_SQ));
    fe_sub(n, n, v);                                         // N = c (r - 1)(d - 1)^2 - v, beta 3
    fe w0, w1, w2, w3;
    fe_add(a, s, s);                                         // beta 2
    fe_mul(w0, a, v);                                        // w0 = 2 s v
    fe_mul(w1, n, fe_const(K_SQRT_AD_MINUS_ONE));            // w1 = N sqrt(a d - 1)
    fe_sqr(w3, s);
    fe_sub(w2, one, w3);                                     // w2 = 1 - s^2, beta 3
    w3.v[0] += 1;                                            // w3 = 1 + s^2
    fe_mul(P.X, w0, w3);
    fe_mul(P.Y, w2, w1);
    fe_mul(P.Z, w1, w3);
    fe_mul(P.T, w2, w0);
}

// one half of the 64 hash bytes as a field element: little-endian, bit 255 masked (the field arithmetic takes it mod p)
C25519_DEV void rist_hash_half(fe& t, const u32 (&w)[8])
{
    u32 m[8];
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = w[i];
    m[7] &= 0x7fffffffu;
    fe_from_words(t, m);
}

// ristretto255_FromHash for one element: two MAPs, one complete addition that forms T, ENCODE: three chains
C25519_DEV void rist_from_hash_lane(u32 (&out)[8], const u32 (&lo)[8], const u32 (&hi)[8])
{
    ge_ext P, Q;
    ge_pe q;
    fe t;
    rist_hash_half(t, hi);
    rist_map(Q, t);
    ge_to_pe(q, Q);
    rist_hash_half(t, lo);
    rist_map(P, t);
    ge_add_pe<true>(P, P, q);
    rist_encode<true>(out, P);
}

// e of the rule: the low 255 bits, no clamp
C25519_DEV void rist_scalar(u32 (&e)[8], const u32 (&s)[8]) { group_scalar(e, s, 0u); }

// ristretto255_ScalarMult for one element: out = ENCODE([e] DECODE(pw)) where pw decodes (returns all-ones), zero words where it
// does not (the row walks all the same)
template <int W>
C25519_DEV u32 rist_scalarmult_lane(u32 (&out)[8], const u32 (&sw)[8], const u32 (&pw)[8])
{
    fe X, Y;
    const u32 ok = rist_decode(X, Y, pw, 0u);
    u32 e[8];
    rist_scalar(e, sw);
    ge_ext S;
    ed_group_walk<W>(S, X, Y, e);
    rist_encode<false>(out, S);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] &= ok;
    return ok;
}

// ristretto255_ScalarMultBase for one element: ENCODE([e]B) over the wide comb (cols, stride: ed_group_base_lane)
template <typename ColT>
C25519_DEV void rist_base_lane(u32 (&out)[8], const u32 (&sw)[8], const u32* __restrict__ g_wide, ColT* cols, int stride)
{
    ge_ext S;
    ed_group_base_lane(S, sw, 0u, g_wide, cols, stride);
    rist_encode<false>(out, S);
}

// ristretto255_PointAdd / PointSub for one element: out = ENCODE(P + Q) (negate = zero) or ENCODE(P - Q) (all-ones) where both
// decode (returns all-ones), zero words where one does not
C25519_DEV u32 rist_add_lane(u32 (&out)[8], const u32 (&pw)[8], const u32 (&qw)[8], u32 negate)
{
    // the two decodings as ONE rolled loop over a masked choice of the input and of where the result goes: unrolled, the two
    // square-root chains and the encoding's spilled 20 registers at two waves per SIMD
    fe X, Y, t;
    ge_ext S;
    u32 ok = 0xffffffffu;
    fe_set_u32(S.X, 0);
    fe_set_u32(S.Y, 0);
#pragma unroll 1
    for (u32 j = 0; j < 2; j++) {
        const u32 second = 0u - j;
        u32 w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = (pw[i] & ~second) | (qw[i] & second);
        ok &= rist_decode(X, Y, w, negate & second);
        fe_select(S.X, second, S.X, X);
        fe_select(S.Y, second, S.Y, Y);
    }
    fe_set_u32(S.Z, 1);
    fe_mul(S.T, S.X, S.Y);
    ge_pa A;
    fe_add(t, Y, X);  fe_carry32(A.ypx, t);
    fe_sub(t, Y, X);  fe_carry32(A.ymx, t);
    fe_mul(t, X, Y);
    fe_mul(A.t2d, t, fe_const(K_2D));
    ge_add_pa<true>(S, A);
    rist_encode<true>(out, S);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] &= ok;
    return ok;
}

}  // namespace c25519
