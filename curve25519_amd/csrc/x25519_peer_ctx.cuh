// curve25519_amd/csrc/x25519_peer_ctx.cuh -- X25519 against MANY peer keys in one call (curve25519_dh_Peer_Init_*,
// curve25519_dh_CreateSharedKey_indexed_*): what one lane does to build a peer context, what one lane does per secret against
// the context its index names, and the gather of a context's key for the calls that run the ladder.  engine_x25519.hip wraps
// these in its kernels; tests/host_emul/peer_ctx.cpp drives the same functions on the CPU.
//
// The context (C25519_AMD_PEER_CTX_SIZE = 1600 bytes, include/curve25519_amd.h):
//   words 0..7     the peer key as given            word 8   eligibility (1: the rows stand in for the ladder)
//   words 9..15    zero                             words 16 + 24 r .. 16 + 24 r + 23   row r = Y+X | Y-X | 2dXY, canonical
// Row r = sum over the set bits i of r of 2^(64 i) * Q with Q = 8 P, affine (Z = 1): the 4-fold table of ed25519_Verify_Init
// (qtable_build) for Q instead of -A, in ge_pa form.  The identity and the eligibility are x25519_peer.cuh's: k * P =
// (k >> 3) * Q for a clamped k, Q has order L or 1, and x(k P) leaves as u = (Z + Y) / (Z - Y).  A context of a small-order
// peer has 16 neutral rows: the walk ends on a zero denominator and the shared inversion gives 0, the ladder's answer.
// An ineligible peer (twist, u = -1) gets eligibility 0 and zero rows; its elements run the ladder on the key in words 0..7.
//
// The walk is ge_poly_mult's 4-fold half: 64 columns of k' = k >> 3 (fold4_next: bit i of column n = bit 63 - n of 64-bit limb i),
// one doubling and one mixed addition each.  The secret only selects rows: every column adds its row, row 0 included, and the
// recoding is bit gathering.  The index and the context are public (which peer a secret is for); a context is trusted data.
#pragma once
#include "fe25519.cuh"
#include "ge25519.cuh"
#include "x25519_peer.cuh"

namespace c25519 {

constexpr size_t PEER_CTX_BYTES = 1600, PEER_CTX_WORDS = PEER_CTX_BYTES / 4;
constexpr int PEER_CTX_ELIGIBLE = 8;             // word of the eligibility flag
constexpr int PEER_CTX_ROWS = 16;                // word offset of row 0
constexpr int PEER_ROW_WORDS = 24;
static_assert(PEER_CTX_ROWS + 16 * PEER_ROW_WORDS == (int)PEER_CTX_WORDS, "the rows end the context");

// element i's context, or null when its index is out of range
C25519_DEV const u32* peer_ctx_of(const u32* ctxs, size_t n_ctx, const u32* ctx_index, size_t i)
{
    const u32 k = ctx_index[i];
    return k < n_ctx ? ctxs + (size_t)k * PEER_CTX_WORDS : nullptr;
}

// the key stored in a context; 32 zero bytes for no context (an index >= n_ctx: the ladder on u = 0 gives 0)
C25519_DEV void peer_ctx_key(u32 (&u)[8], const u32* ctx)
{
    if (!ctx) {
#pragma unroll
        for (int j = 0; j < 8; j++) u[j] = 0;
        return;
    }
    const uint4* p = reinterpret_cast<const uint4*>(ctx);
    const uint4 a = p[0], b = p[1];
    u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w; u[4] = b.x; u[5] = b.y; u[6] = b.z; u[7] = b.w;
}

C25519_DEV void peer_ctx_put_words(u32* dst, const u32 (&w)[8])
{
    uint4* p = reinterpret_cast<uint4*>(dst);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// curve25519_dh_Peer_Init for one key u: the 1600-byte context to `ctx`.  `tbl` is lane-private scratch of QTABLE_LIMB_WORDS
// words (the projective rows before normalisation).  The 15 rows share ONE inversion (Montgomery's trick); the prefix products
// wait in the row slots of the context itself, each overwritten by its final row on the way back.
C25519_DEV void peer_ctx_build(u32* ctx, const u32 (&u)[8], u32* tbl)
{
    u32 w[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    peer_ctx_put_words(ctx, u);
    u32 q[3][8];
    const bool ok = x25519_peer_point(q, u) != 0;
    w[0] = ok ? 1u : 0u;
    peer_ctx_put_words(ctx + 8, w);                      // eligibility, then seven zero words
    w[0] = 0;
    u32* rows = ctx + PEER_CTX_ROWS;
    if (!ok) {                                           // (the key is public: so is its eligibility)
#pragma unroll 1
        for (int r = 0; r < 16 * 3; r++) peer_ctx_put_words(rows + 8 * r, w);
        return;
    }
    ge_pa pa;
    x25519_peer_pa(pa, &q[0][0]);
    ge_ext Q;
    ge_from_pa(Q, pa);                                   // (2x, 2y, 2, 2xy)
    const QTableLimbs t{ tbl };
    qtable_build(t, Q);                                  // rows 0..15 as (Y+X, Y-X, 2dT, 2Z)
    ge_pe pe;
    fe acc, z;
#pragma unroll 1
    for (int r = 1; r < 16; r++) {                       // prefix products of 2Z over rows 1..r, parked in row r's slot
        t.load(pe, (u32)r);
        if (r == 1) acc = pe.z2; else fe_mul(acc, acc, pe.z2);
        fe_to_words(w, acc);
        peer_ctx_put_words(rows + PEER_ROW_WORDS * r, w);
    }
    fe inv;
    fe_invert(inv, acc);                                 // 1 / (2Z_1 ... 2Z_15): never zero, Q is a point of the curve
#pragma unroll 1
    for (int r = 15; r >= 1; r--) {
        fe zi, s, f;
        t.load(pe, (u32)r);
        if (r > 1) {
            const uint4* p = reinterpret_cast<const uint4*>(rows + PEER_ROW_WORDS * (r - 1));
            const uint4 a = p[0], b = p[1];
            const u32 pw[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
            fe_from_words(z, pw);
            fe_mul(zi, inv, z);                          // 1 / 2Z_r
            fe_mul(inv, inv, pe.z2);
        } else {
            zi = inv;
        }
        fe_add(f, zi, zi);
        fe_carry32(s, f);                                // 1 / Z_r
        u32* row = rows + PEER_ROW_WORDS * r;
        fe_mul(f, pe.ypx, s);  fe_to_words(w, f);  peer_ctx_put_words(row, w);
        fe_mul(f, pe.ymx, s);  fe_to_words(w, f);  peer_ctx_put_words(row + 8, w);
        fe_mul(f, pe.t2d, s);  fe_to_words(w, f);  peer_ctx_put_words(row + 16, w);
    }
    const u32 one[8] = { 1, 0, 0, 0, 0, 0, 0, 0 }, zero[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    peer_ctx_put_words(rows, one);                       // row 0: the neutral element
    peer_ctx_put_words(rows + 8, one);
    peer_ctx_put_words(rows + 16, zero);
}

// row r of a context's table (`rows` = ctx + PEER_CTX_ROWS), limbs from its canonical words (any 256-bit words: fe_from_words)
C25519_DEV void peer_ctx_row(ge_pa& q, const u32* __restrict__ rows, u32 r)
{
    const uint4* p = reinterpret_cast<const uint4*>(rows + (size_t)r * PEER_ROW_WORDS);
    const uint4 a0 = p[0], a1 = p[1], b0 = p[2], b1 = p[3], c0 = p[4], c1 = p[5];
    const u32 wa[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
    const u32 wb[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
    const u32 wc[8] = { c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w };
    fe_from_words(q.ypx, wa);
    fe_from_words(q.ymx, wb);
    fe_from_words(q.t2d, wc);
}

// the 64 4-fold columns of k' = k >> 3 (k = the CLAMPED scalar words) in walk order, eight 4-bit columns per word, to cols[j * stride]
// (j = 0..7): fold4_next's bit gathering done once, so that the walk holds one word of them at a time instead of k'
C25519_DEV void peer_ctx_columns(u32* cols, int stride, const u32 (&k)[8])
{
    u32 k3[8];                                           // k >> 3: exact, the three low bits are clear
#pragma unroll
    for (int i = 0; i < 7; i++) k3[i] = (k[i] >> 3) | (k[i + 1] << 29);
    k3[7] = k[7] >> 3;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        u32 w = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) w |= fold4_next(k3, j >= 4) << (4 * c);
        cols[j * stride] = w;
    }
}

// one secret against one context's rows, its columns parked by peer_ctx_columns.  The numerator and denominator of
// u = (Z + Y) / (Z - Y), for the shared inversion (FinishX25519).
C25519_DEV void peer_ctx_walk(fe& num, fe& den, const u32* cols, int stride, const u32* __restrict__ rows)
{
    ge_pa q;
    ge_ext S;
    peer_ctx_row(q, rows, cols[0] & 15u);
    ge_from_pa(S, q);
#pragma unroll 1
    for (int n = 1; n < 64; n++) {
        ge_double<true>(S);
        peer_ctx_row(q, rows, (cols[(n >> 3) * stride] >> (4 * (n & 7))) & 15u);
        C25519_SCHED_FENCE();
        ge_add_pa<false>(S, q);                          // a doubling follows: it does not read T
    }
    fe t;
    fe_add(t, S.Z, S.Y);  fe_carry32(num, t);
    fe_sub(t, S.Z, S.Y);  fe_carry32(den, t);
}

}  // namespace c25519
