// curve25519_amd/csrc/sc_invert.cuh -- the scalar field's lane functions (ed25519_Scalar*_*: engine_scalar.hip): 1/s mod L (the
// base-point order) by Bernstein-Yang division steps, Montgomery's trick over K elements per lane, and the element-wise calls.
//
// A Fermat chain s^(L-2) over sc_mul is ~252 squarings and a dozen products of ~64 multiply-adds plus sc_reduce512's ~250
// instructions each: on the order of 85 000 instructions.  safegcd25519.cuh inverts mod p in ~16 000 by 20 batches of 30 division
// steps, and only two of its functions know the modulus: the update of the cofactors d, e (the multiple of the modulus that makes
// the division by 2^30 exact) and the final normalisation.  Those two are written here for L; sg_divsteps30, sg_update_fg,
// sg_from_words and sg_to_words are used as they are.
//   * f starts as L, g as the input reduced to [0, L) (sc_mod); zeta = -1.  The bound the header cites -- 590 steps for moduli below
//     2^256 -- covers the 253-bit L, so 20 batches leave g = 0, f = +-1 and 1/s = sign(f) d.
//   * L = 2^252 + c, c < 2^125: in 30-bit limbs (K_L_LIMBS30) limbs 0..4 hold c, limbs 5..7 are zero, limb 8 is 2^12 -- six
//     multiply-adds by the multiple md per number and batch where p = (-19, 0, ..., 0, 2^15) needed two.
//   * Bounds of a column of sc_update_de: |u d_i + v e_i| <= 2^60 (|u| + |v| <= 2^30 for a batch's matrix, limbs below 2^30; the top
//     limb of d, e in (-2L, L) is below 2^14), md in (-2^31, 2^30] times a limb of L below 2^30 is below 2^61, the carry is below
//     2^33: under 2^62, the accumulator is signed 64-bit.  The CPU model counts any wrap (valu_model.h: mad_i64_i32).
// Plain C++ with masks only: no branch and no address depends on a scalar's value.  The only decisions are on the public element
// index (is this slot of the group inside the call?).
#pragma once
#include "sc25519.cuh"
#include "lanes.cuh"

namespace c25519 {

// (d, e) <- (t (d, e) + L (md, me)) / 2^30 with md, me chosen to make the division exact; d, e stay in (-2L, L)
C25519_DEV void sc_update_de(sg30& d, sg30& e, const sg_mat& t)
{
    const i32 sd = d.v[8] >> 31, se = e.v[8] >> 31;      // a negative d (e) adds its matrix column to the multiple of L
    i32 md = (t.u & sd) + (t.v & se);
    i32 me = (t.q & sd) + (t.r & se);
    i64 cd = mad2_i64_i32(0, t.u, d.v[0], t.v, e.v[0]);
    i64 ce = mad2_i64_i32(0, t.q, d.v[0], t.r, e.v[0]);
    md -= (i32)((K_L_INV30 * (u32)cd + (u32)md) & (u32)SG_M30);
    me -= (i32)((K_L_INV30 * (u32)ce + (u32)me) & (u32)SG_M30);
    cd = mad_i64_i32(cd, K_L_LIMBS30[0], md);
    ce = mad_i64_i32(ce, K_L_LIMBS30[0], me);
    cd >>= 30;  ce >>= 30;
#pragma unroll
    for (int i = 1; i < 9; i++) {
        cd = mad2_i64_i32(cd, t.u, d.v[i], t.v, e.v[i]);
        ce = mad2_i64_i32(ce, t.q, d.v[i], t.r, e.v[i]);
        if (i <= 4 || i == 8) { cd = mad_i64_i32(cd, K_L_LIMBS30[i], md);  ce = mad_i64_i32(ce, K_L_LIMBS30[i], me); }
        d.v[i - 1] = (i32)cd & SG_M30;  cd >>= 30;
        e.v[i - 1] = (i32)ce & SG_M30;  ce >>= 30;
    }
    d.v[8] = (i32)cd;
    e.v[8] = (i32)ce;
}

// d in (-2L, L), negated where sign < 0, to [0, L) with limbs in [0, 2^30)
C25519_DEV void sc_normalize(sg30& d, i32 sign)
{
    i32 add = d.v[8] >> 31;                              // negative: + L
    const i32 neg = sign >> 31;
#pragma unroll
    for (int i = 0; i < 9; i++) d.v[i] += K_L_LIMBS30[i] & add;
#pragma unroll
    for (int i = 0; i < 9; i++) d.v[i] = (d.v[i] ^ neg) - neg;
#pragma unroll
    for (int i = 0; i < 8; i++) { d.v[i + 1] += d.v[i] >> 30;  d.v[i] &= SG_M30; }
    add = d.v[8] >> 31;                                  // still negative (it was in (-2L, -L], or the negation made it so): + L
#pragma unroll
    for (int i = 0; i < 9; i++) d.v[i] += K_L_LIMBS30[i] & add;
#pragma unroll
    for (int i = 0; i < 8; i++) { d.v[i + 1] += d.v[i] >> 30;  d.v[i] &= SG_M30; }
}

// out = 1 / in mod L as canonical words; in: any 256-bit value.  0 mod L -> 0.
C25519_DEV void sc_invert_words(u32 (&out)[8], const u32 (&in)[8])
{
    u32 x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = in[i];
    sc_mod(x);
    sg30 f, g, d, e;
    sg_from_words(g, x);
#pragma unroll
    for (int i = 0; i < 9; i++) { f.v[i] = K_L_LIMBS30[i]; d.v[i] = 0; e.v[i] = 0; }
    e.v[0] = 1;
    i32 zeta = -1;
#pragma unroll 1
    for (int it = 0; it < 20; it++) {
        sg_mat t;
        zeta = sg_divsteps30(zeta, (u32)f.v[0] | ((u32)f.v[1] << 30), (u32)g.v[0] | ((u32)g.v[1] << 30), t);
        sc_update_de(d, e, t);
        sg_update_fg(f, g, t);
    }
    // g = 0 and f = +-1 now (+-L for in = 0, where d = 0): 1/in = sign(f) d
    sc_normalize(d, f.v[8]);
    sg_to_words(out, d);
}

// all-ones where the eight words are not all zero
C25519_DEV u32 sc_nonzero_mask(const u32 (&x)[8])
{
    u32 any = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) any |= x[i];
    return (u32)0 - ((any | ((u32)0 - any)) >> 31);
}

// slot j of a lane's group for the shared inversion, as loaded: the lane's element j, or zero where the slot is past the call's end
// (a decision on the public index).  group: the lane's first element; j is a compile-time constant where the loops are unrolled, so
// the address is the lane's one base register pair and an immediate offset -- sixteen slots' addresses computed up front are 32
// registers the K = 16 kernel does not have ...
C25519_DEV void sc_invert_slot_load(u32 (&x)[8], const void* group, int j, bool inside)
{
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = 0;
    if (inside) load32(x, group, (size_t)j);
}
// A line the compiler moves neither memory accesses nor the computation of x across (no instruction), and at which the eight
// words of x stand in eight registers (left alone it keeps some zero-extended to the 64 bits the next product reads them as).
// The lane's loads do not depend on its arithmetic: left alone the compiler issues all K slots' loads in front of the first product, 128 registers at
// K = 16 that two waves per SIMD do not leave.  The CPU model needs no such line and gets none (an asm output would also read as
// initialised to MemorySanitizer and hide the word from the secret-taint run).
#if defined(__HIP_DEVICE_COMPILE__)
C25519_DEV void sc_order_line(u32 (&x)[8])
{
    __asm__ volatile("" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]) : : "memory");
}
#else
C25519_DEV void sc_order_line(u32 (&)[8]) {}
#endif

// ... and as the products take it: mod L, zero (a missing slot too) swapped for one.  Returns all-ones where it was not zero.
C25519_DEV u32 sc_invert_slot_prepare(u32 (&x)[8])
{
    sc_mod(x);
    const u32 nz = sc_nonzero_mask(x);
    x[0] |= ~nz & 1u;
    return nz;
}

// What one lane of k_sc25519_invert<K> does: elements lane K .. lane K + K - 1 of the call (the ragged tail's missing slots count as
// one) by Montgomery's trick -- prefix products forward, ONE sc_invert_words, back-substitution: three sc_mul per element.  The
// K - 1 prefix products the way back needs stay in registers (the loops over the K slots are fully unrolled) -- at K = 16 all but
// the first sc_invert_parked<K>() of them, which wait in LDS (word w of product j at park[(8 j + w) stride]: 48 KiB per workgroup of 256
// lanes; the 120 registers of fifteen products beside a product's working set do not fit the 256 of two waves per SIMD, the
// compiler spilled 40 of them).  An element itself is not kept: the way back loads it again.  Both passes issue a slot's load one
// slot ahead of the products that use it; the scheduling fences and sc_order_line keep the compiler from interleaving the slots'
// loads and products.  The way back loads slot j - 1 before the lane stores slot j, and a lane touches its own slots only -- so
// recip may be s itself.  A zero takes no part (swapped for one), its output is forced to zero and ok says so.
template <int K>
constexpr int sc_invert_parked() { return K > 8 ? 6 : 0; }

template <int K>
C25519_DEV void sc_invert_lane(void* recip, int* ok, const void* s, size_t n, size_t lane, u32* park, int stride)
{
    constexpr int PARK = sc_invert_parked<K>();
    const size_t e0 = lane * K;
    const void* s_group = (const unsigned char*)s + 32 * e0;
    void* recip_group = (unsigned char*)recip + 32 * e0;
    int* ok_group = ok + e0;
    const int slots = n - e0 < (size_t)K ? (int)(n - e0) : K;         // how many of the group's slots the call has (the caller: e0 < n)
    u32 pre[K - PARK][8], cur[8], t[8], next[8], inv[8];              // pre[j - PARK]: the product of slots 0 .. j
    u32 nzbits = 0;
    sc_invert_slot_load(next, s_group, 0, true);
#pragma unroll
    for (int j = 0; j < K; j++) {
#pragma unroll
        for (int w = 0; w < 8; w++) t[w] = next[w];
        if (j + 1 < K) sc_invert_slot_load(next, s_group, j + 1, j + 1 < slots);
        nzbits |= (sc_invert_slot_prepare(t) & 1u) << j;
        if (j == 0) {
#pragma unroll
            for (int w = 0; w < 8; w++) cur[w] = t[w];
        } else {
            sc_mul(cur, cur, t);
        }
        if (j < PARK) {
#pragma unroll
            for (int w = 0; w < 8; w++) park[(8 * j + w) * stride] = cur[w];
        } else {
#pragma unroll
            for (int w = 0; w < 8; w++) pre[j - PARK][w] = cur[w];
        }
        C25519_SCHED_FENCE();
        sc_order_line(cur);
    }
    sc_invert_words(inv, cur);
    sc_order_line(inv);
    if (K > 1) sc_invert_slot_load(next, s_group, K - 1, K - 1 < slots);
#pragma unroll
    for (int j = K - 1; j >= 0; j--) {
        u32 r[8];
        if (j > 0) {
#pragma unroll
            for (int w = 0; w < 8; w++) t[w] = next[w];
            if (j > 1) sc_invert_slot_load(next, s_group, j - 1, j - 1 < slots);
            sc_invert_slot_prepare(t);
            if (j - 1 < PARK) {
#pragma unroll
                for (int w = 0; w < 8; w++) cur[w] = park[(8 * (j - 1) + w) * stride];
                sc_mul(r, inv, cur);
            } else {
                sc_mul(r, inv, pre[j - 1 - PARK]);
            }
            C25519_SCHED_FENCE();
            sc_mul(inv, inv, t);
        } else {
#pragma unroll
            for (int w = 0; w < 8; w++) r[w] = inv[w];
        }
        const u32 m = (u32)0 - ((nzbits >> j) & 1u);
#pragma unroll
        for (int w = 0; w < 8; w++) r[w] &= m;
        if (j < slots) {
            store32(recip_group, (size_t)j, r);
            ok_group[j] = (int)(m & 1u);
        }
        C25519_SCHED_FENCE();
        sc_order_line(inv);
    }
}

// r = L - y for y in [0, L]: in [0, L]
C25519_DEV void sc_l_minus(u32 (&r)[8], const u32 (&y)[8])
{
    u32 borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 d = (u64)K_L[i] - y[i] - borrow;
        r[i] = (u32)d;
        borrow = (u32)(d >> 63);
    }
}

// 1 where s < L, else 0
C25519_DEV u32 sc_is_canonical(const u32 (&s)[8])
{
    u32 borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 d = (u64)s[i] - K_L[i] - borrow;
        borrow = (u32)(d >> 63);
    }
    return borrow;
}

// the element-wise calls: one lane per element, `op` uniform over the call.  Every input is any 256-bit value (Reduce: 512-bit),
// every output the canonical representative: sc_mul and sc_reduce512 end canonical, sc_add ends on 256 bits and sc_mod finishes.
enum ScOp { SC_OP_REDUCE = 0, SC_OP_ADD, SC_OP_SUB, SC_OP_MUL, SC_OP_NEGATE, SC_OP_COMPLEMENT, SC_OP_MULADD, SC_OP_COUNT };

C25519_DEV void sc_op_lane(int op, void* r, const void* a, const void* b, const void* c, size_t i)
{
    u32 x[8], y[8], z[8];
    switch (op) {
    case SC_OP_REDUCE: {                                  // a: n x 64 bytes, rows 2 i and 2 i + 1 of 32
        u32 t[16];
        load32(x, a, 2 * i);
        load32(y, a, 2 * i + 1);
#pragma unroll
        for (int w = 0; w < 8; w++) { t[w] = x[w]; t[8 + w] = y[w]; }
        sc_reduce512(z, t);
        break;
    }
    case SC_OP_ADD:
        load32(x, a, i);
        load32(y, b, i);
        sc_add(z, x, y);
        sc_mod(z);
        break;
    case SC_OP_SUB:                                       // x + (L - y mod L)
        load32(x, a, i);
        load32(y, b, i);
        sc_mod(y);
        sc_l_minus(y, y);
        sc_add(z, x, y);
        sc_mod(z);
        break;
    case SC_OP_MUL:
        load32(x, a, i);
        load32(y, b, i);
        sc_mul(z, x, y);
        break;
    case SC_OP_NEGATE:                                    // L - s mod L, and L -> 0
        load32(x, a, i);
        sc_mod(x);
        sc_l_minus(z, x);
        sc_mod(z);
        break;
    case SC_OP_COMPLEMENT: {                              // (L - s mod L) + 1 <= L + 1
        load32(x, a, i);
        sc_mod(x);
        sc_l_minus(z, x);
        u64 carry = 1;
#pragma unroll
        for (int w = 0; w < 8; w++) { carry += z[w];  z[w] = (u32)carry;  carry >>= 32; }
        sc_mod(z);
        break;
    }
    default: {                                            // SC_OP_MULADD: a b + c
        u32 p[8];
        load32(x, a, i);
        load32(y, b, i);
        sc_mul(p, x, y);
        load32(x, c, i);
        sc_add(z, p, x);
        sc_mod(z);
        break;
    }
    }
    store32(r, i, z);
}

}  // namespace c25519
