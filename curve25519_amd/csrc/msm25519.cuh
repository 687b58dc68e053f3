// curve25519_amd/csrc/msm25519.cuh -- what one LANE does in each stage of the ZIP-215 batch equation (engine_batch_eq.hip):
//     T = [sum z_i s_i mod L] B + sum [z_i] (-R_i) + sum [z_i k_i mod L] (-A_i),     result = ([8] T == O) and no element rejected
// as ONE bucket-method multi-scalar multiplication over the 2n decoded points plus one walk of the wide base comb.
//   scalars   k_i = H(R || A || m) mod L, z_i = first 16 bytes of SHA-512(seed || le64(i)), a_i = z_i k_i, s_i = z_i S_i (mod L)
//   points    ed_zip215_decode, negated, stored as ONE packed 128-byte row (Y+X | Y-X | 2dXY | pad): no window tables
//   digits    signed c-bit digits of a scalar, read from its BIASED form: with 2^(c-1) added into every window but the top one,
//             digit w = window w of the biased scalar - 2^(c-1) (the top one as it is), so every digit is independent of the others
//             (no carry chain across windows), |digit| <= 2^(c-1).  The top window of a scalar holds few distinct digits (a_i < L:
//             2^t + 1 of them), so its entries would pile up in a few buckets and one lane each would add 2^20 / 33 rows in sequence;
//             there a bucket is split by point index into G = buckets / R sub-buckets, R = 2^(t+1): slot = |digit| - 1 + R * (point mod G),
//             and slot s stands for the digit (s mod R) + 1.  The top window of the z_i gets a window of its own for that (index wa)
//   buckets   one lane per (window, bucket): the sum of the rows its list names (ge_add_pa; a negative digit flips the row)
//   windows   sum_d d * Bucket_d by running sums over a chunk of buckets, chunks joined by a short multiply with the chunk's offset
//   tail      Horner over the windows, + [s] B, then the hook's encoding or three doublings and the neutral test
// The coalesced form (ed25519_VerifyBatch_zip215_indexed_*: n elements over K keys, N = K + n points) sums the canonical a_i of a key's
// elements first (msm_scalars_canonical, integer sums per 32-bit word, msm_key_fold) and gives the key ONE scalar; every later stage is
// the same code over fewer points.
// The kernels add the cross-lane parts (counting sort with atomics, reductions); the CPU emulator (tests/host_emul/verify_batch.cpp)
// drives the same functions with a host counting sort in between.  The a = -1 unified additions are complete on the curve, so equal
// points, P + (-P) and the small-order points of the conformance grid take the same code as everything else.
#pragma once
#include "lanes.cuh"
#include "verify_fast.cuh"
#include "coop_ops.cuh"

namespace c25519 {

constexpr int MSM_C_MIN = 7, MSM_C_MAX = 13;                // window widths the kernels take (2^(c-1) buckets: 64 .. 4096 per window)
constexpr int MSM_ROW_WORDS = 32;                           // one point: a packed 128-byte line, as a row of the wide comb
constexpr int MSM_EXT_WORDS = 40;                           // a bucket / window sum: X, Y, Z, T as limbs

// windows of a scalar below 2^bits: the top window stays unbiased and must hold its value plus a carry within 2^(c-1)
constexpr int msm_windows(int bits, int c) { return (bits + 2 + c - 1) / c; }
constexpr int msm_windows_a(int c) { return msm_windows(253, c); }      // a_i < L < 2^253
constexpr int msm_windows_z(int c) { return msm_windows(128, c); }      // z_i < 2^128
// log2 R of a top window: a scalar below 2^bound (+ less than one unit of the top window) has top digits 0 .. 2^t + 1, t = bound - c (nwin - 1)
constexpr int msm_top_rlog2(int bound, int c, int nwin) { return (bound - c * (nwin - 1) > 0 ? bound - c * (nwin - 1) : 0) + 1; }

// the shape of one equation: c, the windows of a key's and of an R's scalar, 2^(c-1) buckets per window, and log2 R of the two top
// windows.  There are wa + 1 windows of buckets: 0 .. wa - 1 by position, and wa = the z_i's top window (position wz - 1).
struct MsmShape { int c, wa, wz, buckets, ra, rz; };
constexpr MsmShape msm_shape(int c)
{
    return MsmShape{ c, msm_windows_a(c), msm_windows_z(c), 1 << (c - 1), msm_top_rlog2(252, c, msm_windows_a(c)),     // a_i < L < 2^252 + 2^125
                     msm_top_rlog2(128, c, msm_windows_z(c)) };
}
C25519_DEV int msm_window_rlog2(const MsmShape& sh, int w) { return w == sh.wa ? sh.rz : w == sh.wa - 1 ? sh.ra : sh.c - 1; }
// which digit of point p's scalar (-1: none) goes into bucket window w
C25519_DEV int msm_window_digit(const MsmShape& sh, int w, bool is_r)
{
    if (!is_r) return w < sh.wa ? w : -1;
    return w == sh.wa ? sh.wz - 1 : w < sh.wz - 1 ? w : -1;
}
// the slot of window w's buckets an entry goes to
C25519_DEV u32 msm_slot(const MsmShape& sh, int w, int absd, u32 p)
{
    const int rl = msm_window_rlog2(sh, w), r = 1 << rl;
    return (u32)((absd < r ? absd : r) - 1) + ((p & (u32)((sh.buckets >> rl) - 1)) << rl);
}

// k += 2^(c-1) in every window below the top one.  k < 2^253 and c * (nwin - 1) < 255: the sum stays below 2^256.
C25519_DEV void msm_bias(u32 (&k)[8], int c, int nwin)
{
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        u32 b = 0;
        for (int w = 0; w < nwin - 1; w++) {
            const int bit = w * c + c - 1;
            b |= (bit >> 5) == j ? 1u << (bit & 31) : 0u;
        }
        carry += (u64)k[j] + b;
        k[j] = (u32)carry;
        carry >>= 32;
    }
}

// digit w of the biased scalar whose word j sits at sc[j * stride]
C25519_DEV int msm_digit(const u32* sc, size_t stride, int w, int c, int nwin)
{
    const int bit = w * c, j = bit >> 5;
    const u32 lo = j < 8 ? sc[(size_t)j * stride] : 0u, hi = j + 1 < 8 ? sc[(size_t)(j + 1) * stride] : 0u;
    const u32 v = (u32)(pair64(lo, hi) >> (bit & 31)) & ((1u << c) - 1u);
    return (int)v - (w < nwin - 1 ? 1 << (c - 1) : 0);
}

// z_i: one compression, the 40-byte string seed || le64(index) with its padding laid out by hand
C25519_DEV void msm_challenge(u32 (&z)[8], const u32 (&seedw)[8], u64 index)
{
    u64 st[8] = { 0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                  0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull };
    u64 w[16];
    sha512_words_from_le32(w, seedw);
    w[4] = be64_from_le32((u32)index, (u32)(index >> 32));
    w[5] = 0x8000000000000000ull;
#pragma unroll
    for (int j = 6; j < 15; j++) w[j] = 0;
    w[15] = 40 * 8;
    sha512_compress(st, w);
    u32 le[16];
    sha512_digest_le_words(le, st);
#pragma unroll
    for (int j = 0; j < 8; j++) z[j] = j < 4 ? le[j] : 0u;
}

// the scalars of one element: a = z k mod L and s = z S mod L, both CANONICAL, and z BIASED for width c.  Returns all-ones iff S < L.
C25519_DEV u32 msm_scalars_canonical(u32 (&a)[8], u32 (&z)[8], u32 (&s)[8], const u32 (&pkw)[8], const u32 (&Rw)[8], const u32 (&Sw)[8],
                                     const uint8_t* msg, size_t len, const u32 (&seedw)[8], u64 index, int c)
{
    u32 k[8];
    ed_hram(k, Rw, pkw, msg, len);
    sc_mod(k);
    msm_challenge(z, seedw, index);
    sc_mul(a, z, k);
    sc_mod(a);
    sc_mul(s, z, Sw);
    sc_mod(s);
    msm_bias(z, c, msm_windows_z(c));
    return zip215_pair_flags(Sw) ? 0u : 0xffffffffu;
}

// stage 1 for one element: a = z k mod L and z, both BIASED for width c; s = z S mod L (canonical).  Returns all-ones iff S < L.
C25519_DEV u32 msm_scalars(u32 (&a)[8], u32 (&z)[8], u32 (&s)[8], const u32 (&pkw)[8], const u32 (&Rw)[8], const u32 (&Sw)[8],
                           const uint8_t* msg, size_t len, const u32 (&seedw)[8], u64 index, int c)
{
    const u32 ok = msm_scalars_canonical(a, z, s, pkw, Rw, Sw, msg, len, seedw, index, c);
    msm_bias(a, c, msm_windows_a(c));
    return ok;
}

// the coalesced equation (ed25519_VerifyBatch_zip215_indexed_*), one key: the eight 64-bit sums of its elements' a_i, word by word
// (each sum below 2^58: at most 2^26 elements), -> their total mod L, BIASED for width c.  Returns all-ones iff the total is not zero
// (a key with total zero has no digits: nobody named it, or only rejected elements did, or its terms cancel).
C25519_DEV u32 msm_key_fold(u32 (&a)[8], const u64 (&sum)[8], int c)
{
    u32 t[16];
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        carry += j < 8 ? sum[j] : 0ull;
        t[j] = (u32)carry;
        carry >>= 32;
    }
    sc_reduce512(a, t);
    sc_mod(a);
    u32 any = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) any |= a[j];
    msm_bias(a, c, msm_windows_a(c));
    return any ? 0xffffffffu : 0u;
}

// stage 2 for one point: the packed row of -P.  Returns all-ones iff the string decodes.
C25519_DEV u32 msm_point_row(u32 (&row)[24], const u32 (&enc)[8])
{
    fe X, Y, t;
    const u32 ok = ed_zip215_decode(X, Y, enc, 0xffffffffu);
    u32 w[8];
    fe_add(t, Y, X);  fe_carry32(t, t);  fe_to_words(w, t);
#pragma unroll
    for (int j = 0; j < 8; j++) row[j] = w[j];
    fe_sub(t, Y, X);  fe_carry32(t, t);  fe_to_words(w, t);
#pragma unroll
    for (int j = 0; j < 8; j++) row[8 + j] = w[j];
    fe_mul(t, X, Y);
    fe_mul(t, t, fe_const(K_2D));
    fe_to_words(w, t);
#pragma unroll
    for (int j = 0; j < 8; j++) row[16 + j] = w[j];
    return ok;
}

// the row an entry of the inverted index names: entry = point index * 2 + (1: the digit was negative, add the point's negative)
C25519_DEV void msm_load_row(ge_pa& q, const u32* __restrict__ rows, u32 entry)
{
    const u32 neg = 0u - (entry & 1u);
    const uint4* r = reinterpret_cast<const uint4*>(rows + (size_t)(entry >> 1) * MSM_ROW_WORDS);
    const uint4* p_ypx = r + (neg ? 2 : 0);                  // a negated point swaps Y+X and Y-X ...
    const uint4* p_ymx = r + (neg ? 0 : 2);
    const uint4 a0 = p_ypx[0], a1 = p_ypx[1], b0 = p_ymx[0], b1 = p_ymx[1], c0 = r[4], c1 = r[5];
    const u32 wa[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
    const u32 wb[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
    const u32 wc[8] = { c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w };
    fe t, n;
    fe_from_words(q.ypx, wa);
    fe_from_words(q.ymx, wb);
    fe_from_words(t, wc);
    fe_neg(n, t);                                            // ... and negates 2dxy
    fe_select(q.t2d, neg, n, t);
}

C25519_DEV void msm_set_neutral(ge_ext& S)
{
    fe_set_u32(S.X, 0); fe_set_u32(S.Y, 1); fe_set_u32(S.Z, 1); fe_set_u32(S.T, 0);
}

C25519_DEV void msm_store_ext(u32* p, const ge_ext& S)
{
    const fe* f[4] = { &S.X, &S.Y, &S.Z, &S.T };
    uint4* row = reinterpret_cast<uint4*>(p);
    u32 w[MSM_EXT_WORDS];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 10; i++) w[10 * j + i] = f[j]->v[i];
#pragma unroll
    for (int g = 0; g < 10; g++) row[g] = make_uint4(w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]);
}

C25519_DEV void msm_load_ext(ge_ext& S, const u32* p)
{
    fe* f[4] = { &S.X, &S.Y, &S.Z, &S.T };
    const uint4* row = reinterpret_cast<const uint4*>(p);
    u32 w[MSM_EXT_WORDS];
#pragma unroll
    for (int g = 0; g < 10; g++) {
        const uint4 v = row[g];
        w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 10; i++) f[j]->v[i] = w[10 * j + i];
}

// r += q, both extended with T
C25519_DEV void msm_ext_add(ge_ext& r, const ge_ext& q)
{
    ge_pe pe;
    ge_to_pe(pe, q);
    ge_add_pe<true>(r, r, pe);
}

// stage 4 for one bucket: the sum of the rows entries[begin .. end) name
C25519_DEV void msm_bucket_sum(ge_ext& S, const u32* __restrict__ rows, const u32* __restrict__ entries, u32 begin, u32 end)
{
    msm_set_neutral(S);
#pragma unroll 1
    for (u32 i = begin; i < end; i++) {
        ge_pa q;
        msm_load_row(q, rows, entries[i]);
        C25519_SCHED_FENCE();
        ge_add_pa<true>(S, q);
    }
}

// stage 5 for one chunk of a window's buckets: sum over slots b in [lo, hi) of ((b mod R) + 1) * Bucket_b, R = 2^rlog2 (a power of two,
// like hi - lo and lo / (hi - lo)).  Running sums from the top of the chunk give sum (b - lo + 1) Bucket_b and run = sum Bucket_b, and
// (lo mod R) * run joins the chunk to its run of R slots (double-and-add over the offset's bits); where the chunk holds several such runs
// the running sum starts again at the top of each and the offset is 0.
C25519_DEV void msm_chunk_sum(ge_ext& acc, const u32* __restrict__ buckets, u32 lo, u32 hi, int rlog2)
{
    const u32 rmask = (1u << rlog2) - 1u;
    ge_ext run, t;
    msm_set_neutral(run);
    msm_set_neutral(acc);
#pragma unroll 1
    for (u32 b = hi; b > lo; b--) {
        if (((b - 1) & rmask) == rmask) msm_set_neutral(run);
        msm_load_ext(t, buckets + (size_t)(b - 1) * MSM_EXT_WORDS);
        msm_ext_add(run, t);
        msm_ext_add(acc, run);
    }
    lo &= rmask;
    if (lo == 0) return;
    ge_pe pe;
    ge_to_pe(pe, run);
    msm_set_neutral(t);
#pragma unroll 1
    for (int bit = MSM_C_MAX - 2; bit >= 0; bit--) {         // lo < 2^(MSM_C_MAX - 1)
        ge_double<true>(t);
        if ((lo >> bit) & 1u) ge_add_pe<true>(t, t, pe);
    }
    msm_ext_add(acc, t);
}

// stage 6, first part: T = sum_w 2^(c w) Window_w, the z_i's top window (index wa) at position wz - 1
C25519_DEV void msm_horner(ge_ext& T, const u32* __restrict__ windows, const MsmShape& sh)
{
    ge_ext t;
    msm_load_ext(T, windows + (size_t)(sh.wa - 1) * MSM_EXT_WORDS);
#pragma unroll 1
    for (int w = sh.wa - 2; w >= 0; w--) {
#pragma unroll 1
        for (int j = 0; j < sh.c - 1; j++) ge_double<false>(T);
        ge_double<true>(T);
        msm_load_ext(t, windows + (size_t)w * MSM_EXT_WORDS);
        msm_ext_add(T, t);
        if (w == sh.wz - 1) {
            msm_load_ext(t, windows + (size_t)sh.wa * MSM_EXT_WORDS);
            msm_ext_add(T, t);
        }
    }
}

// the 16 sixteen-bit chunk sums of the elements' s_i (each below 2^48) -> their total mod L, canonical
C25519_DEV void msm_fold_s(u32 (&s)[8], const u64 (&chunk)[16])
{
    u32 h[32], t[16];
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 32; j++) {
        carry += j < 16 ? chunk[j] : 0ull;
        h[j] = (u32)carry & 0xffffu;
        carry >>= 16;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) t[j] = h[2 * j] | (h[2 * j + 1] << 16);
    sc_reduce512(s, t);
    sc_mod(s);
}

// stage 6, the end: enc(T) for the hook ...
C25519_DEV void msm_encode(u32 (&enc)[8], const ge_ext& T)
{
    u32 xw[8], yw[8];
    ge_to_affine_words(xw, yw, T);
    ge_pack(enc, xw, yw);
}

// ... or [8] T == O: X == 0 and Y == Z (Z != 0 under the complete law).  T is consumed.
C25519_DEV u32 msm_times8_is_neutral(ge_ext& T)
{
#pragma unroll 1
    for (int j = 0; j < 3; j++) ge_double<false>(T);
    u32 xw[8], dw[8], acc = 0;
    fe d;
    fe_sub(d, T.Y, T.Z);
    fe_to_words(xw, T.X);
    fe_to_words(dw, d);
#pragma unroll
    for (int i = 0; i < 8; i++) acc |= xw[i] | dw[i];
    return acc == 0 ? 0xffffffffu : 0u;
}

}  // namespace c25519
