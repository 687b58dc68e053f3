// curve25519_amd/csrc/ed_keys.cuh -- what ONE lane does for the key calls (include/curve25519_amd.h states their rules):
//   ed25519_ClassifyKey_*             the four flag bits of a 32-byte Ed25519 key
//   ed25519_PublicKey_to_X25519_*     u = (1 + y) / (1 - y) of a key that decodes, is not of small order and is torsion-free
//   ed25519_PrivateKey_to_X25519_*    the clamped first half of SHA-512(seed)
// engine_keys.hip wraps these in its key kernels; tests/host_emul/key_convert.cpp drives the same functions on the CPU.
//
// The new work is the walk [L]A for a variable point A: the library's other walks either run over tables built for a fixed point or
// carry a secret or per-element scalar.  L is public and the same in every lane, so its digits are compile-time data: L in signed
// binary non-adjacent form (K_L_NAF_NZ / K_L_NAF_NEG, tools/gen_constants.py) has the digit +1 at bit 252 and 45 digits +-1 below
// bit 125, no two adjacent.  The lane keeps A alone, in affine precomputed form, and flips it for a digit -1 as msm_load_row flips
// a row (Y+X and Y-X trade places, 2dXY is negated): 252 doublings and 45 mixed additions, no table, no lane-private scratch.  A
// doubling does not read T, and a non-zero digit is always followed by a zero one, so only the doubling in front of an addition
// forms T and no addition does.  The loop's branches test bits of the two constant masks at a wave-uniform index: no lane diverges.
// Public data only: nothing here needs to be constant-time, except ed_key_private_to_x25519, which has no branch on its data.
#pragma once
#include "lanes.cuh"
#include "strict25519.cuh"
#include "verify_fast.cuh"

namespace c25519 {

constexpr u32 KEY_DECODES = 1u, KEY_CANONICAL = 2u, KEY_SMALL_ORDER = 4u, KEY_TORSION_FREE = 8u;    // C25519_AMD_KEY_*

// all-ones iff S is the neutral element: X == 0 and Y == Z (Z != 0 for a curve point under the complete law)
C25519_DEV u32 ge_is_neutral(const ge_ext& S)
{
    u32 xw[8], dw[8], acc = 0;
    fe d;
    fe_sub(d, S.Y, S.Z);
    fe_to_words(xw, S.X);
    fe_to_words(dw, d);
#pragma unroll
    for (int i = 0; i < 8; i++) acc |= xw[i] | dw[i];
    return acc == 0 ? 0xffffffffu : 0u;
}

// S = [L](x, y) for affine x, y with reduced limbs; T of the result is not formed
C25519_DEV void ed_key_walk_L(ge_ext& S, const fe& x, const fe& y)
{
    ge_pa A;
    fe t;
    fe_add(t, y, x);  fe_carry32(A.ypx, t);
    fe_sub(t, y, x);  fe_carry32(A.ymx, t);
    fe_mul(t, x, y);
    fe_mul(A.t2d, t, fe_const(K_2D));
    S.X = x;                                                 // digit 252 is +1
    S.Y = y;
    fe_set_u32(S.Z, 1);
#pragma unroll 1
    for (int i = 251; i >= 0; i--) {
        const u32 nz = (K_L_NAF_NZ[i >> 5] >> (i & 31)) & 1u;
        if (!nz) {
            ge_double<false>(S);
            continue;
        }
        ge_double<true>(S);
        const u32 neg = 0u - ((K_L_NAF_NEG[i >> 5] >> (i & 31)) & 1u);
        ge_pa q;
        fe_select(q.ypx, neg, A.ymx, A.ypx);
        fe_select(q.ymx, neg, A.ypx, A.ymx);
        fe_neg(t, A.t2d);                                    // 2p - 2dxy: beta 2, fine as the second factor of a product
        fe_select(q.t2d, neg, t, A.t2d);
        ge_add_pa<false>(S, q);
    }
}

// the flags of the key bytes w; X, Y: the decoded point (what the decoder left where the bytes do not decode)
C25519_DEV u32 ed_key_classify(fe& X, fe& Y, const u32 (&w)[8])
{
    const u32 decodes = ed_zip215_decode(X, Y, w, 0u);
    u32 yw[8], xw[8], x_bits = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) yw[i] = w[i];
    yw[7] &= 0x7fffffffu;
    fe_to_words(xw, X);
#pragma unroll
    for (int i = 0; i < 8; i++) x_bits |= xw[i];
    const u32 zero_x_signed = (x_bits == 0 && (w[7] >> 31)) ? decodes : 0u;
    const u32 canonical = strict_less(yw, K_P) & ~zero_x_signed;
    const u32 small = strict_small_y(w) & decodes;
    ge_ext S;
    ed_key_walk_L(S, X, Y);                                  // (a key that does not decode walks too: the bit is masked)
    const u32 torsion_free = ge_is_neutral(S) & decodes;
    return (decodes & KEY_DECODES) | (canonical & KEY_CANONICAL) | (small & KEY_SMALL_ORDER) | (torsion_free & KEY_TORSION_FREE);
}

// all-ones where ed25519_PublicKey_to_X25519 accepts a key with these flags
C25519_DEV u32 ed_key_converts(u32 flags)
{
    return (flags & (KEY_DECODES | KEY_SMALL_ORDER | KEY_TORSION_FREE)) == (KEY_DECODES | KEY_TORSION_FREE) ? 0xffffffffu : 0u;
}

// numerator and denominator of u = (1 + y) / (1 - y) for the shared inversion, reduced; returns ed_key_converts of the key's flags.
// den = 0 only for y = 1, the neutral element, which is of small order.
C25519_DEV u32 ed_key_to_x25519_lane(fe& num, fe& den, const u32 (&w)[8])
{
    fe X, Y, one, t;
    const u32 ok = ed_key_converts(ed_key_classify(X, Y, w));
    fe_set_u32(one, 1);
    fe_add(t, one, Y);  fe_carry32(num, t);
    fe_sub(t, one, Y);  fe_carry32(den, t);
    return ok;
}

// the shared inversion's output for ed25519_PublicKey_to_X25519: xpk = canonical(num / den) where the element's ok word is set,
// 32 zero bytes where it is not
struct FinishKeyX25519 {
    const u32 *num, *ok; void* out; size_t n;
    C25519_DEV bool skip() const { return false; }
    C25519_DEV void emit(size_t e, const fe& zinv) const
    {
        fe x;
        u32 w[8];
        soa_load_fe(x, num, n, e);
        fe_mul(x, x, zinv);
        fe_to_words(w, x);
        const u32 keep = ok[e];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] &= keep;
        store32(out, e, w);
    }
};

// ed25519_PrivateKey_to_X25519 for element e: SHA-512 of the seed half of the 64-byte privKey (one compression), first half, clamped
C25519_DEV void ed_key_private_to_x25519(void* xsk, const void* priv, size_t e)
{
    u32 seed[8], a[8];
    u64 b_words[4];
    load32(seed, priv, 2 * e);
    ed_expand_seed(a, b_words, seed);
    store32(xsk, e, a);
}

}  // namespace c25519
