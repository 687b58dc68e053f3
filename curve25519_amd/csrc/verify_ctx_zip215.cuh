// curve25519_amd/csrc/verify_ctx_zip215.cuh -- the ZIP-215 verdict against Verify_Init contexts (ed25519_Verify_Check_zip215_*,
// ed25519_Verify_Check_zip215_indexed_*) WITHOUT decoding R.  The context kernels (engine_verify_ctx.hip: k_ed25519_verify_check_indexed,
// _shared, _wide -- launched as the plain calls launch them) leave T = [S]B - [k]A projectively in scratch.  ZIP-215's rule 4,
// [8](T - R) = O, says that R lies in the coset T + E[8], E[8] the eight points of small order.  So with y_R = (the low 255 bits of
// R's string) mod p and sign = bit 255, rules 3 (R decodes) and 4 hold exactly when one of the eight points C = T + t has
//     y_C = y_R   and   (x_C = 0  or  parity(x_C) = sign):
// a y that is the y of a curve point has its square root, the sign bit picks between x_C and -x_C (and is ignored for x = 0), and a
// string that does not decode, or decodes outside the coset, matches none of the eight.  No square root, no doublings.
//
// The eight candidates for T = (x, y) = (X / Z, Y / Z), i = sqrt(-1), (x8, y8) a point of order 8, c = d x y x8 y8:
//     +-(x, y)   +-(i y, i x)                                                      -- T + the four points of order <= 4 --
//     +-((x y8 + y x8) / (1 + c), (y y8 + x x8) / (1 - c))   +-((x y8 - y x8) / (1 - c), (y y8 - x x8) / (1 + c))
// and 1 +- c = (Z^2 +- k X Y) / Z^2 with the constant k = d x8 y8, so ONE inversion of W = Z (Z^2 + kXY)(Z^2 - kXY) per element -- the
// shared one, k_batch_invert pointed at W -- gives 1 / Z and Z / (Z^2 +- kXY) with a few products.  The curve's law is complete: W is
// not zero for a curve point.  A zero W (a context that is not Verify_Init's, or the zero point an index out of range leaves) gets
// verdict 0.  Per element: 5 products in coset_prep_element, 21 and 9 canonicalisations in FinishVerifyZip215 (it rebuilds the two
// denominators: 3 products, against 20 more words of scratch per element), against ~1 200 products of the walk in front.
//
// Rule 2 (the key decodes) is decided once per context, not per pair (zip215_ctx_key_ok): Verify_Init decodes the key with the
// function ZIP-215 uses (ge_calc_x: y mod p, x = 0 whatever the sign bit), and row 1 of its context holds -A as (y + x, y - x, 2dxy, 2).
// ge_calc_x's x satisfies the curve equation with y exactly when the key decodes, so the equation on row 1's (x, y), and row 1's y
// being the key's y mod p, IS rule 2 for a context that is Verify_Init's: 4 products per context instead of a square root.
// Rule 1 (S < L) is applied where the verdict is written.
//
// Everything the comparison reads -- R, S, the index -- is public; it is written without divergent exits all the same, because the
// lanes of a wave see different inputs.  In a header of its own so that tests/host_emul compiles it too
// (tests/host_emul/verify_check_zip215.cpp); tests/check_zip215_model.py is the same algebra in big integers, and derives the constants.
#pragma once
#include "verify_ctx.cuh"
#include "strict25519.cuh"

namespace c25519 {

// a point of order 8, (x8, y8), and k = d x8 y8
__device__ constexpr uint32_t K_T8X[8] = { 0xc545d14au, 0xdea14646u, 0x13e5e238u, 0x5c193c70u, 0x38de4abbu, 0xe9339932u, 0x06394a28u, 0x1fd5b9a0u };
__device__ constexpr uint32_t K_T8Y[8] = { 0x706a17c7u, 0x4fd84d3du, 0x760b3cbau, 0x0f67100du, 0xfa53202au, 0xc6cc392cu, 0x77fdc74eu, 0x7a03ac92u };
__device__ constexpr uint32_t K_T8K[8] = { 0x9389cecbu, 0x438611c7u, 0xc8a83936u, 0xdee0a612u, 0x6ff1a9a4u, 0x3a89fd62u, 0x7b4527b7u, 0x62ec563fu };

// dp = Z^2 + kXY (beta 2), dm = Z^2 - kXY (beta 3).  X, Y, Z reduced.
C25519_DEV void coset_denominators(fe& dp, fe& dm, const fe& X, const fe& Y, const fe& Z)
{
    fe zz, kxy;
    fe_sqr(zz, Z);
    fe_mul(kxy, X, Y);
    fe_mul(kxy, kxy, fe_const(K_T8K));
    fe_add(dp, zz, kxy);
    fe_sub(dm, zz, kxy);
}

// element e of the coset prep: W = Z (Z^2 + kXY)(Z^2 - kXY) into the scratch part the shared inversion is then pointed at
C25519_DEV void coset_prep_element(u32* W, const u32* X, const u32* Y, const u32* Z, size_t n, size_t e)
{
    fe x, y, z, dp, dm, w;
    soa_load_fe(x, X, n, e);
    soa_load_fe(y, Y, n, e);
    soa_load_fe(z, Z, n, e);
    coset_denominators(dp, dm, x, y, z);
    fe_mul(w, dm, dp);
    fe_mul(w, w, z);
    soa_store_fe(W, n, e, w);
}

// rule 2 for the context at `ctx` (see above): 1 or 0
C25519_DEV u32 zip215_ctx_key_ok(const u32* ctx)
{
    u32 w[8];
    fe ypx, ymx, yk, x2, y2, xx, yy, t, u;
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = ctx[j];
    w[7] &= 0x7fffffffu;
    fe_from_words(yk, w);
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = ctx[8 + 32 + j];
    fe_from_words(ypx, w);
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = ctx[8 + 32 + 8 + j];
    fe_from_words(ymx, w);
    fe_sub(x2, ypx, ymx);                                  // 2x, beta 3
    fe_add(y2, ypx, ymx);                                  // 2y, beta 2
    // -x^2 + y^2 = 1 + d x^2 y^2, times 16:  4 ((2y)^2 - (2x)^2) = 16 + d (2x)^2 (2y)^2
    fe_sqr(xx, x2);
    fe_sqr(yy, y2);
    fe_sub(t, yy, xx);                                     // beta 3
    fe_mul_small(t, t, 4);
    fe_mul(u, xx, yy);
    fe_mul(u, u, fe_const(K_D));
    u.v[0] += 16;
    fe_sub(t, t, u);
    u32 cw[8], diff = 0;
    fe_to_words(cw, t);
#pragma unroll
    for (int j = 0; j < 8; j++) diff |= cw[j];
    // ... and row 1's y is the key's:  2y = 2 y_key
    fe_add(u, yk, yk);
    fe_carry32(u, u);
    fe_sub(t, y2, u);
    fe_to_words(cw, t);
#pragma unroll
    for (int j = 0; j < 8; j++) diff |= cw[j];
    return diff == 0 ? 1u : 0u;
}

// y_R = (the low 255 bits of Rw) mod p and p - y_R (0 for y_R = 0), canonical words; returns the sign bit
C25519_DEV u32 zip215_r_words(u32 (&yr)[8], u32 (&yrn)[8], const u32 (&Rw)[8])
{
    u32 v[8], red[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = Rw[j];
    v[7] &= 0x7fffffffu;
    u64 c = 19;                                            // v - p = v + 19 - 2^255
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += v[j];
        red[j] = (u32)c;
        c >>= 32;
    }
    red[7] &= 0x7fffffffu;
    const u32 below = strict_less(v, K_P);
    u32 nz = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        yr[j] = (v[j] & below) | (red[j] & ~below);
        nz |= yr[j];
    }
    const u32 keep = nz ? 0xffffffffu : 0u;
    u32 borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const u64 d = (u64)K_P[j] - yr[j] - borrow;
        yrn[j] = (u32)d & keep;
        borrow = (u32)(d >> 63);
    }
    return Rw[7] >> 31;
}

// does (cx, cy) or (-cx, -cy) match (y_R, sign)?  1 or 0.  cx, cy: any beta fe_to_words takes
C25519_DEV u32 coset_match(const fe& cx, const fe& cy, const u32 (&yr)[8], const u32 (&yrn)[8], u32 sign)
{
    u32 xw[8], yw[8], dpos = 0, dneg = 0, xnz = 0;
    fe_to_words(xw, cx);
    fe_to_words(yw, cy);
#pragma unroll
    for (int j = 0; j < 8; j++) {
        dpos |= yw[j] ^ yr[j];
        dneg |= yw[j] ^ yrn[j];                            // -y = y_R  <=>  y = p - y_R (0 for 0)
        xnz |= xw[j];
    }
    const u32 par = xw[0] & 1u;                            // x != 0: parity(-x) = 1 - parity(x), p being odd
    const u32 pos = (dpos == 0 ? 1u : 0u) & ((xnz == 0 ? 1u : 0u) | (par == sign ? 1u : 0u));
    const u32 neg = (dneg == 0 ? 1u : 0u) & ((xnz == 0 ? 1u : 0u) | (par != sign ? 1u : 0u));
    return pos | neg;
}

// rules 3 and 4 for T = (X : Y : Z) given w_inv = 1 / (Z (Z^2 + kXY)(Z^2 - kXY)), 0 for a zero product: 1 or 0
C25519_DEV u32 coset_contains_r(const fe& X, const fe& Y, const fe& Z, const fe& w_inv, const u32 (&Rw)[8])
{
    u32 yr[8], yrn[8], ww[8], wnz = 0;
    const u32 sign = zip215_r_words(yr, yrn, Rw);
    fe_to_words(ww, w_inv);
#pragma unroll
    for (int j = 0; j < 8; j++) wnz |= ww[j];
    fe dp, dm, t, z_inv, zdp, zdm;
    coset_denominators(dp, dm, X, Y, Z);
    fe_mul(t, dm, dp);
    fe_mul(z_inv, t, w_inv);                               // 1 / Z
    fe_mul(t, w_inv, Z);
    fe_mul(t, t, Z);
    fe_mul(zdp, dm, t);                                    // Z / (Z^2 + kXY)
    fe_mul(zdm, dp, t);                                    // Z / (Z^2 - kXY)
    fe x, y, cx, cy;
    fe_mul(x, X, z_inv);
    fe_mul(y, Y, z_inv);
    u32 hit = coset_match(x, y, yr, yrn, sign);            // +-(x, y)
    fe_mul(cx, y, fe_const(K_SQRTM1));
    fe_mul(cy, x, fe_const(K_SQRTM1));
    hit |= coset_match(cx, cy, yr, yrn, sign);             // +-(i y, i x)
    fe a, b, c, e;
    fe_mul(a, X, fe_const(K_T8Y));
    fe_mul(b, Y, fe_const(K_T8X));
    fe_mul(c, Y, fe_const(K_T8Y));
    fe_mul(e, X, fe_const(K_T8X));
    fe_add(t, a, b);  fe_mul(cx, t, zdp);                  // beta 2
    fe_add(t, c, e);  fe_mul(cy, t, zdm);
    hit |= coset_match(cx, cy, yr, yrn, sign);             // +-(T + (x8, y8))
    fe_sub(t, a, b);  fe_mul(cx, t, zdm);                  // beta 3
    fe_sub(t, c, e);  fe_mul(cy, t, zdp);
    hit |= coset_match(cx, cy, yr, yrn, sign);             // +-(T + (-x8, y8))
    return hit & (wnz ? 1u : 0u);
}

// k_batch_invert's finish: the inversion ran over W (coset_prep_element); verdict = rules 1-4 and the element's index in range.
// ctx_index null: one context for the whole call (key_ok[0]).
struct FinishVerifyZip215 {
    const u32 *X, *Y, *Z; const void* sig; int* verdict; size_t n;
    const u32* ctx_index; size_t n_ctx;
    const u32* key_ok;                                     // one word per context: zip215_ctx_key_ok
    C25519_DEV bool skip() const { return false; }
    C25519_DEV void emit(size_t e, const fe& w_inv) const
    {
        fe x, y, z;
        u32 Rw[8], Sw[8];
        soa_load_fe(x, X, n, e);
        soa_load_fe(y, Y, n, e);
        soa_load_fe(z, Z, n, e);
        load32(Rw, sig, 2 * e);
        load32(Sw, sig, 2 * e + 1);
        const u32 k = ctx_index ? ctx_index[e] : 0u;
        const u32 in_range = k < n_ctx ? 1u : 0u;
        const u32 key = key_ok[in_range ? k : 0u];
        const u32 hit = coset_contains_r(x, y, z, w_inv, Rw);
        verdict[e] = (int)(hit & in_range & key & (strict_less(Sw, K_L) & 1u));
    }
};

}  // namespace c25519
