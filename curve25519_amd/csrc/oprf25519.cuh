// curve25519_amd/csrc/oprf25519.cuh -- what ONE lane does for RFC 9497's OPRF (mode 0x00) and VOPRF (mode 0x01) with ciphersuite
// ristretto255-SHA512 (include/curve25519_amd.h states the calls' rules):
//   ristretto255_OPRF_Blind_*            blind * HashToGroup(input)                                  (3.3.1 Blind, 3.3.2 Blind)
//   ristretto255_OPRF_Finalize_*         SHA-512(lp(input) || lp((1 / blind) * evaluated) || "Finalize")   (3.3.1 Finalize, 3.3.2 after VerifyProof)
//   ristretto255_OPRF_BlindEvaluate_*    skS * blinded under ONE key                                 (3.3.1 BlindEvaluate)
//   ristretto255_VOPRF_BlindEvaluate_*   the same with a DLEQ proof per request                      (3.3.2 BlindEvaluate, 2.2.1 GenerateProof)
//   ristretto255_VOPRF_VerifyProof_*     2.2.2 VerifyProof per request
// engine_oprf.hip wraps these in its kernels; tests/host_emul/oprf.cpp drives the same functions on the CPU.
//
// Nothing new in the field or the group: the lane strings together the pieces the other calls have.
//   * HashToGroup: the expander of h2c25519.cuh under "HashToGroup-" || contextString, the two Elligator maps of ristretto255.cuh and
//     their sum -- which goes into the walk as it stands, extended and projective: the window table is built from it (oprf_table), no
//     ENCODE and no DECODE in between (two inverse-square-root chains fewer than HashToGroup_dev + ScalarMult_dev).
//   * The walks are ed_group.cuh's masked walk at width 2 (its recoding, its selection) over a table built once per point: in the
//     server's row lane skS and then d_i walk the table of C_i.
//   * The short hashes have fixed lengths: the composite seed (69 bytes), d_i's expander input (145) and the challenge's (179) are laid
//     out at compile time (OprfFrame) with the lane's 32- and 64-byte fields ORed in at constant offsets; both expansions are
//     Z_pad's constant, two blocks, and one block for b_1.  Finalize's string begins with two length bytes and then the input, so
//     nothing in it is word aligned: the input is read by bytes and the 43 bytes behind it are shifted into place by a uniform amount.
//   * Which request a row belongs to is found by bisection over `offsets` (oprf_owner).  Every size read from there is checked before
//     it bounds a loop or forms an index; an array that does not rise from 0 to n gives requests without rows and rows without a
//     request, never an access outside the call's arrays.
// Secret: input, blind and what is derived from them up to `blinded` and `output`; skS; proof_rand (r), t2, t3 before the challenge is
// formed and r - c skS.  Public: blinded, evaluated, pkS, the composites' seed, d_i, M, Z, c, s.  No branch and no address depends on a
// secret but the comb's row fetch for [skS]B and [r]B (wb_load_pa_signed, as in signing); the verdicts that depend on a secret being
// zero mod L are formed and applied as masks (tests/host_emul/taint_oprf.cpp).
// Limb bounds (fe25519.cuh's contract): every value named below is reduced unless a comment gives its beta.
#pragma once
#include "ed_group.cuh"
#include "h2c25519.cuh"
#include "sc_invert.cuh"

namespace c25519 {

constexpr int OPRF_DIGITS = GroupWindow<2>::DIGITS;          // 129 signed two-bit digits of a scalar below 2^255
constexpr int OPRF_GROUP_DST_LEN = 40, OPRF_SCALAR_DST_LEN = 41, OPRF_SEED_DST_LEN = 33;
constexpr u32 OPRF_MAX_ROWS = 65535;                         // of one proof: the row index is I2OSP(i, 2)
constexpr u32 OPRF_NO_OWNER = 0xffffffffu;
constexpr int OPRF_HEAD_WORDS = 32;                          // a call's public header in scratch: pkS (8 words), the composites' seed (16 words)

// "HashToGroup-" || "OPRFV1-" || mode || "-ristretto255-SHA512", on the HOST
inline void oprf_group_dst(unsigned char (&dst)[OPRF_GROUP_DST_LEN], unsigned mode)
{
    const char s[] = "HashToGroup-OPRFV1-?-ristretto255-SHA512";
    static_assert(sizeof s == OPRF_GROUP_DST_LEN + 1, "40 characters");
    for (int i = 0; i < OPRF_GROUP_DST_LEN; i++) dst[i] = (unsigned char)s[i];
    dst[19] = (unsigned char)mode;
}

// the uniform part of a Blind call's HashToGroup, on the HOST
inline void oprf_make_tail(H2cTail& t, size_t input_size, unsigned mode)
{
    unsigned char dst[OPRF_GROUP_DST_LEN];
    oprf_group_dst(dst, mode);
    h2c_make_tail(t, input_size, dst, OPRF_GROUP_DST_LEN, 64);
}

// ---- strings of a fixed layout as the big-endian words SHA-512 takes ----------------------------------------------------------
template <int WORDS> struct OprfFrame { u64 w[WORDS]; };

template <int WORDS>
C25519_DEV constexpr void oprf_frame_byte(OprfFrame<WORDS>& f, int k, unsigned byte) { f.w[k / 8] |= (u64)byte << (56 - 8 * (k % 8)); }
template <int WORDS>
C25519_DEV constexpr int oprf_frame_text(OprfFrame<WORDS>& f, int k, const char* s)
{
    for (int i = 0; s[i]; i++) oprf_frame_byte(f, k++, (unsigned char)s[i]);
    return k;
}
// "<label>OPRFV1-" || 0x01 || "-ristretto255-SHA512" from byte k
template <int WORDS>
C25519_DEV constexpr int oprf_frame_dst(OprfFrame<WORDS>& f, int k, const char* label)
{
    k = oprf_frame_text(f, k, label);
    k = oprf_frame_text(f, k, "OPRFV1-");
    oprf_frame_byte(f, k++, 0x01);
    return oprf_frame_text(f, k, "-ristretto255-SHA512");
}
// the end of a hashed string of `total` bytes that lies behind `before` hashed bytes: 0x80 and the bit length in the last word
template <int WORDS>
C25519_DEV constexpr void oprf_frame_close(OprfFrame<WORDS>& f, int total, int before)
{
    oprf_frame_byte(f, total, 0x80);
    f.w[WORDS - 1] = (u64)(before + total) << 3;
}
// b_0's input behind Z_pad for a message of LEN bytes under HashToScalar's DST: msg || I2OSP(64, 2) || 0x00 || DST || 0x29
template <int LEN> struct OprfXmd {
    static constexpr int TOTAL = LEN + 3 + OPRF_SCALAR_DST_LEN + 1;
    static constexpr int WORDS = 16 * ((TOTAL + 17 + 127) / 128);
};
template <int LEN>
C25519_DEV constexpr void oprf_frame_xmd(OprfFrame<OprfXmd<LEN>::WORDS>& f)
{
    oprf_frame_byte(f, LEN + 1, 64);
    int k = oprf_frame_dst(f, LEN + 3, "HashToScalar-");
    oprf_frame_byte(f, k++, OPRF_SCALAR_DST_LEN);
    oprf_frame_close(f, k, 128);
}

constexpr int OPRF_COMPOSITE_LEN = 2 + 64 + 2 + 34 + 34 + 9, OPRF_CHALLENGE_LEN = 5 * 34 + 9;
using OprfCompositeFrame = OprfFrame<OprfXmd<OPRF_COMPOSITE_LEN>::WORDS>;
using OprfChallengeFrame = OprfFrame<OprfXmd<OPRF_CHALLENGE_LEN>::WORDS>;
static_assert(OprfXmd<OPRF_COMPOSITE_LEN>::WORDS == 32 && OprfXmd<OPRF_CHALLENGE_LEN>::WORDS == 32, "two blocks each behind Z_pad");

// lp(seed) || I2OSP(i, 2) || lp(C_i) || lp(D_i) || "Composite": the constant bytes
C25519_DEV constexpr OprfCompositeFrame oprf_composite_frame()
{
    OprfCompositeFrame f{};
    oprf_frame_byte(f, 1, 64);
    oprf_frame_byte(f, 69, 32);
    oprf_frame_byte(f, 103, 32);
    oprf_frame_text(f, 136, "Composite");
    oprf_frame_xmd<OPRF_COMPOSITE_LEN>(f);
    return f;
}
// lp(pkS) || lp(M) || lp(Z) || lp(t2) || lp(t3) || "Challenge"
C25519_DEV constexpr OprfChallengeFrame oprf_challenge_frame()
{
    OprfChallengeFrame f{};
    for (int j = 0; j < 5; j++) oprf_frame_byte(f, 34 * j + 1, 32);
    oprf_frame_text(f, 170, "Challenge");
    oprf_frame_xmd<OPRF_CHALLENGE_LEN>(f);
    return f;
}
// b_1's input behind the 64 bytes of b_0: 0x01 || DST || 0x29
C25519_DEV constexpr OprfFrame<16> oprf_b1_frame()
{
    OprfFrame<16> f{};
    oprf_frame_byte(f, 64, 1);
    int k = oprf_frame_dst(f, 65, "HashToScalar-");
    oprf_frame_byte(f, k++, OPRF_SCALAR_DST_LEN);
    oprf_frame_close(f, k, 0);
    return f;
}
// lp(pkS) || lp("Seed-" || contextString)
C25519_DEV constexpr OprfFrame<16> oprf_seed_frame()
{
    OprfFrame<16> f{};
    oprf_frame_byte(f, 1, 32);
    oprf_frame_byte(f, 35, OPRF_SEED_DST_LEN);
    const int k = oprf_frame_dst(f, 36, "Seed-");
    oprf_frame_close(f, k, 0);
    return f;
}

// the 32 bytes v (little-endian words as they sit in memory) at byte OFF of the big-endian word array w
template <int OFF>
C25519_DEV void oprf_put32(u64* w, const u32 (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 be = __builtin_bswap32(v[i]);
        const int o = OFF + 4 * i, k = o / 8, sh = 32 - 8 * (o % 8);
        if (sh >= 0) {
            w[k] |= be << sh;
        } else {
            w[k] |= be >> (-sh);
            w[k + 1] |= be << (64 + sh);
        }
    }
}
C25519_DEV void oprf_sha512_init(u64 (&st)[8])
{
    const u64 iv[8] = { 0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                        0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull };
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = iv[i];
}

// HashToScalar of the two-block string w (an OprfXmd layout with the lane's fields in place): canonical out.  w is consumed.
C25519_DEV void oprf_hash_to_scalar(u32 (&out)[8], u64 (&w)[32])
{
    constexpr OprfFrame<16> B1 = oprf_b1_frame();
    u64 st[8], blk[16];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = K_SHA512_ZPAD_MID[i];
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = w[i];
    sha512_compress(st, blk);
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = w[16 + i];
    sha512_compress(st, blk);
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = i < 8 ? st[i] : B1.w[i];
    oprf_sha512_init(st);
    sha512_compress(st, blk);
    u32 h[16];
    sha512_digest_le_words(h, st);
    sc_reduce512(out, h);
}

// seed = SHA-512(lp(pkS) || lp("Seed-" || contextString)) as digest words
C25519_DEV void oprf_composite_seed(u64 (&seed)[8], const u32 (&pkw)[8])
{
    constexpr OprfFrame<16> F = oprf_seed_frame();
    u64 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = F.w[i];
    oprf_put32<2>(w, pkw);
    oprf_sha512_init(seed);
    sha512_compress(seed, w);
}

// d_i = HashToScalar(lp(seed) || I2OSP(idx, 2) || lp(C_i) || lp(D_i) || "Composite"), idx < 2^16
C25519_DEV void oprf_composite_scalar(u32 (&d)[8], const u64 (&seed)[8], u32 idx, const u32 (&Cw)[8], const u32 (&Dw)[8])
{
    constexpr OprfCompositeFrame F = oprf_composite_frame();
    u64 w[32];
#pragma unroll
    for (int i = 0; i < 32; i++) w[i] = F.w[i];
#pragma unroll
    for (int i = 0; i < 8; i++) {                            // the seed's 64 bytes from byte 2
        w[i] |= seed[i] >> 16;
        w[i + 1] |= seed[i] << 48;
    }
    w[8] |= (u64)(idx & 0xffffu) << 32;                      // bytes 66, 67
    oprf_put32<70>(w, Cw);
    oprf_put32<104>(w, Dw);
    oprf_hash_to_scalar(d, w);
}

// c = HashToScalar(lp(pkS) || lp(M) || lp(Z) || lp(t2) || lp(t3) || "Challenge")
C25519_DEV void oprf_challenge(u32 (&c)[8], const u32 (&pkw)[8], const u32 (&Mw)[8], const u32 (&Zw)[8], const u32 (&t2w)[8], const u32 (&t3w)[8])
{
    constexpr OprfChallengeFrame F = oprf_challenge_frame();
    u64 w[32];
#pragma unroll
    for (int i = 0; i < 32; i++) w[i] = F.w[i];
    oprf_put32<2>(w, pkw);
    oprf_put32<36>(w, Mw);
    oprf_put32<70>(w, Zw);
    oprf_put32<104>(w, t2w);
    oprf_put32<138>(w, t3w);
    oprf_hash_to_scalar(c, w);
}

// ---- points -------------------------------------------------------------------------------------------------------------------
// all-ones where the eight words are not all zero (a ristretto255 encoding: not the identity)
C25519_DEV u32 oprf_nonzero(const u32 (&w)[8]) { return sc_nonzero_mask(w); }

// (x, y) as an extended point with Z = 1
C25519_DEV void oprf_affine_ext(ge_ext& P, const fe& X, const fe& Y)
{
    P.X = X;
    P.Y = Y;
    fe_set_u32(P.Z, 1);
    fe_mul(P.T, X, Y);
}

// rows 1P and 2P of a walk's table; P extended, with T
C25519_DEV void oprf_table(ge_pe (&rows)[2], const ge_ext& P)
{
    ge_ext Q;
    ge_to_pe(rows[0], P);
    ge_add_pe<true>(Q, P, rows[0]);
    ge_to_pe(rows[1], Q);
}

// S = [e]P over P's table, e < 2^255; T of the result is not formed: ed_group_walk<2> from the table on
C25519_DEV void oprf_walk(ge_ext& S, const ge_pe (&rows)[2], const u32 (&e)[8])
{
    u32 t[9];
    group_recode<2>(t, e);
    fe_set_u32(S.X, 0);
    fe_set_u32(S.Y, 1);
    fe_set_u32(S.Z, 1);
    fe_set_u32(S.T, 0);
#pragma unroll 1
    for (int i = 0; i < OPRF_DIGITS; i++) {
        ge_double<false>(S);
        ge_double<true>(S);
        ge_pe q;
        group_select<2>(q, rows, group_next_field<2>(t));
        ge_add_pe<false>(S, S, q);
    }
}

// the same point with T: (X Z, Y Z, Z^2, X Y)
C25519_DEV void oprf_form_t(ge_ext& S)
{
    fe_mul(S.T, S.X, S.Y);
    fe_mul(S.X, S.X, S.Z);
    fe_mul(S.Y, S.Y, S.Z);
    fe_sqr(S.Z, S.Z);
}

// a 32-byte scalar as the calls read it: the 256 bits mod L, canonical
C25519_DEV void oprf_scalar(u32 (&e)[8], const u32 (&s)[8])
{
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = s[i];
    sc_mod(e);
}

// an extended point in the scratch between the kernels of a call: four field elements, struct of arrays over n rows
struct OprfPoints { u32 *X, *Y, *Z, *T; };
C25519_DEV void oprf_store_point(const OprfPoints& p, size_t n, size_t i, const ge_ext& S)
{
    soa_store_fe(p.X, n, i, S.X);
    soa_store_fe(p.Y, n, i, S.Y);
    soa_store_fe(p.Z, n, i, S.Z);
    soa_store_fe(p.T, n, i, S.T);
}
C25519_DEV void oprf_load_point(ge_ext& S, const OprfPoints& p, size_t n, size_t i)
{
    soa_load_fe(S.X, p.X, n, i);
    soa_load_fe(S.Y, p.Y, n, i);
    soa_load_fe(S.Z, p.Z, n, i);
    soa_load_fe(S.T, p.T, n, i);
}

// ---- the per-row calls ---------------------------------------------------------------------------------------------------------
// ristretto255_OPRF_Blind for one element: out = ENCODE([blind] HashToGroup(input)); returns all-ones where that is not the identity
C25519_DEV u32 oprf_blind_lane(u32 (&out)[8], const uint8_t* input, const H2cTail& t, const u32 (&blind)[8])
{
    ge_ext P, S;
    {
        u64 b1[8], b2[8];
        h2c_uniform<false>(b1, b2, input, t);
        u32 h[16], half[8];
        sha512_digest_le_words(h, b1);
        ge_ext Q;
        ge_pe q;
        fe u;
#pragma unroll
        for (int i = 0; i < 8; i++) half[i] = h[8 + i];
        rist_hash_half(u, half);
        rist_map(Q, u);
        ge_to_pe(q, Q);
#pragma unroll
        for (int i = 0; i < 8; i++) half[i] = h[i];
        rist_hash_half(u, half);
        rist_map(P, u);
        ge_add_pe<true>(P, P, q);
    }
    {
        ge_pe rows[2];
        u32 e[8];
        oprf_table(rows, P);
        oprf_scalar(e, blind);
        oprf_walk(S, rows, e);
    }
    rist_encode<false>(out, S);
    return oprf_nonzero(out);
}

// SHA-512(I2OSP(len, 2) || input || I2OSP(32, 2) || N || "Finalize"), len <= 65535 uniform over the call
C25519_DEV void oprf_finalize_hash(u64 (&dg)[8], const uint8_t* input, size_t len, const u32 (&Nw)[8])
{
    // the 43 bytes behind the input with SHA-512's 0x80, as six words ...
    u64 t[6];
#pragma unroll
    for (int i = 0; i < 6; i++) t[i] = 0;
    t[0] = (u64)32 << 48;
    oprf_put32<2>(t, Nw);
    t[4] |= 0x46696e61ull << 16 | 0x6c69;                    // "Finalize" from byte 34
    t[5] = 0x7a65ull << 48 | (u64)0x80 << 40;
    // ... shifted to where the input ends (a uniform amount): seven words from the word the input ends in
    const size_t head = 2 + len, total = head + 42;
    const u32 rem = (u32)(head & 7u), sh = 8 * rem;
    const size_t mw = head >> 3;
    u64 s[7];
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const u64 cur = k < 6 ? t[k < 6 ? k : 0] : 0, prev = k > 0 ? t[k > 0 ? k - 1 : 0] : 0;
        s[k] = rem ? (cur >> sh) | (prev << ((64 - sh) & 63)) : cur;
    }
    const size_t nblocks = (total + 17 + 127) / 128, last_word = 16 * nblocks - 1;
    // byte q of lp(input)'s beginning: the two length bytes, then the input
    auto head_word = [&](size_t g, u32 count) -> u64 {
        u64 v = 0;
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            const size_t q = 8 * g + j;
            u64 byte = 0;
            if (j < count) byte = q < 2 ? (u64)((len >> (8 * (1 - q))) & 0xffu) : (u64)input[q - 2];
            v = (v << 8) | byte;
        }
        return v;
    };
    oprf_sha512_init(dg);
    u64 w[16];
#pragma unroll 1
    for (size_t blk = 0; blk < nblocks; blk++) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const size_t g = 16 * blk + j;
            u64 v;
            if (g < mw) {
                v = head_word(g, 8);
            } else {
                const size_t d = g - mw;
                v = d == 0 ? head_word(g, rem) : 0;
#pragma unroll
                for (int k = 0; k < 7; k++) v |= d == (size_t)k ? s[k] : 0;
                if (g == last_word) v |= (u64)total << 3;
            }
            w[j] = v;
        }
        sha512_compress(dg, w);
    }
}

// ristretto255_OPRF_Finalize for one element: all-ones where evaluated decodes and is not the identity and blind is not 0 mod L;
// out is zeroed where not
C25519_DEV u32 oprf_finalize_lane(u32 (&out)[16], const uint8_t* input, size_t len, const u32 (&blind)[8], const u32 (&ew)[8])
{
    fe X, Y;
    u32 ok = rist_decode(X, Y, ew, 0u) & oprf_nonzero(ew);
    u32 Nw[8];
    {
        u32 b[8], inv[8];
        oprf_scalar(b, blind);
        ok &= sc_nonzero_mask(b);
        sc_invert_words(inv, b);
        ge_ext S;
        ed_group_walk<2>(S, X, Y, inv);
        rist_encode<false>(Nw, S);
    }
    u64 dg[8];
    oprf_finalize_hash(dg, input, len, Nw);
    sha512_digest_le_words(out, dg);
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] &= ok;
    return ok;
}

// ristretto255_OPRF_BlindEvaluate for one element: out = ENCODE([skS] DECODE(pw)); all-ones where pw decodes and neither it nor the
// result is the identity, zero words where not
C25519_DEV u32 oprf_evaluate_lane(u32 (&out)[8], const u32 (&sks)[8], const u32 (&pw)[8])
{
    fe X, Y;
    u32 ok = rist_decode(X, Y, pw, 0u) & oprf_nonzero(pw);
    u32 e[8];
    oprf_scalar(e, sks);
    ge_ext S;
    ed_group_walk<2>(S, X, Y, e);
    rist_encode<false>(out, S);
    ok &= oprf_nonzero(out);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] &= ok;
    return ok;
}

// ---- the proofs ----------------------------------------------------------------------------------------------------------------
// is request j of `offsets` (m + 1 entries) well formed: 1 .. 65 535 rows inside [0, n]?  lo, count: its first row and how many
C25519_DEV bool oprf_request(size_t& lo, u32& count, const unsigned long long* offsets, size_t j, size_t n)
{
    const unsigned long long a = offsets[j], b = offsets[j + 1];
    const bool good = a < b && b - a <= OPRF_MAX_ROWS && b <= n;
    lo = good ? (size_t)a : 0;
    count = good ? (u32)(b - a) : 0u;
    return good;
}

// the request that owns row i and the row's index in it, or OPRF_NO_OWNER: a bisection over offsets[1 .. m] for the first request
// that ends behind the row -- at most 32 steps over indices in [0, m] whatever the array holds --, kept where that request is well
// formed and holds the row.  For offsets that rise from 0 to n this is the request the row lies in.
C25519_DEV u32 oprf_owner(u32& idx, const unsigned long long* offsets, size_t m, size_t n, size_t i)
{
    size_t lo = 0, hi = m;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (offsets[mid + 1] <= i) lo = mid + 1;
        else hi = mid;
    }
    idx = 0;
    if (lo >= m) return OPRF_NO_OWNER;
    size_t first;
    u32 count;
    if (!oprf_request(first, count, offsets, lo, n) || i < first || i - first >= count) return OPRF_NO_OWNER;
    idx = (u32)(i - first);
    return (u32)lo;
}

// what a call's first kernel leaves in scratch for the others: pkS and the composites' seed (public)
struct OprfHead { u32 pk[8]; u64 seed[8]; };
C25519_DEV void oprf_store_head(u32* head, const OprfHead& h)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        head[i] = h.pk[i];
        head[8 + 2 * i] = (u32)h.seed[i];
        head[9 + 2 * i] = (u32)(h.seed[i] >> 32);
    }
}
C25519_DEV void oprf_load_seed(u64 (&seed)[8], const u32* head)
{
#pragma unroll
    for (int i = 0; i < 8; i++) seed[i] = (u64)head[8 + 2 * i] | ((u64)head[9 + 2 * i] << 32);
}
C25519_DEV void oprf_load_head(OprfHead& h, const u32* head)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        h.pk[i] = head[i];
        h.seed[i] = (u64)head[8 + 2 * i] | ((u64)head[9 + 2 * i] << 32);
    }
}

// stage (a) of the server: pkS = ENCODE([skS]B) over the wide comb, and the seed
template <typename ColT>
C25519_DEV void oprf_server_head_lane(OprfHead& h, const u32 (&sks)[8], const u32* __restrict__ g_wide, ColT* cols, int stride)
{
    u32 e[8];
    oprf_scalar(e, sks);
    wb_columns(cols, stride, e);                             // e + L when even: B has order L
    ge_ext S;
    ge_base_mult_wide(S, g_wide, cols, stride);
    rist_encode<false>(h.pk, S);
    oprf_composite_seed(h.seed, h.pk);
}
// ... and of the verifier: pkS as given
C25519_DEV void oprf_verifier_head_lane(OprfHead& h, const u32 (&pkw)[8])
{
#pragma unroll
    for (int i = 0; i < 8; i++) h.pk[i] = pkw[i];
    oprf_composite_seed(h.seed, h.pk);
}

// A line the compiler does not move the computation of a across and behind which it knows nothing about a's value (no instruction;
// sc_invert.cuh's sc_order_line says why the CPU model gets none): the server's row lane builds C_i's two table rows AGAIN from the
// affine point behind it, an addition, instead of keeping 80 limbs of table alive under the encoding of D_i and the hash -- the
// difference between two waves per SIMD and one.
#if defined(__HIP_DEVICE_COMPILE__)
C25519_DEV void oprf_order_line(fe& a)
{
    __asm__ volatile("" : "+v"(a.v[0]), "+v"(a.v[1]), "+v"(a.v[2]), "+v"(a.v[3]), "+v"(a.v[4]), "+v"(a.v[5]), "+v"(a.v[6]), "+v"(a.v[7]), "+v"(a.v[8]),
                     "+v"(a.v[9]));
}
#else
C25519_DEV void oprf_order_line(fe&) {}
#endif

// rows 1P and 2P for the affine point (x, y)
C25519_DEV void oprf_affine_table(ge_pe (&rows)[2], const fe& X, const fe& Y)
{
    ge_ext P;
    oprf_affine_ext(P, X, Y);
    oprf_table(rows, P);
}

// stage (b) of the server for row i: D_i = [skS]C_i and [d_i]C_i over the table of C_i, decoded ONCE.  load_c(w) / load_seed(seed):
// the row's 32 bytes and the call's seed, fetched where they are needed; Dw: the row's `evaluated` (zero words where rejected); term:
// [d_i]C_i extended with T (some point for a rejected row: its request fails); returns all-ones where the row is accepted: owned,
// decodes, neither it nor D_i the identity
template <typename LoadC, typename LoadSeed>
C25519_DEV u32 oprf_server_row_lane(u32 (&Dw)[8], ge_ext& term, const u32 (&sks)[8], const LoadC& load_c, const LoadSeed& load_seed, u32 idx, u32 owned)
{
    fe X, Y;
    u32 ok = owned;
    {
        u32 Cw[8], e[8];
        load_c(Cw);
        ok &= rist_decode(X, Y, Cw, 0u) & oprf_nonzero(Cw);
        ge_pe rows[2];
        oprf_affine_table(rows, X, Y);
        oprf_scalar(e, sks);
        oprf_walk(term, rows, e);
    }
    oprf_order_line(X);
    oprf_order_line(Y);
    rist_encode<false>(Dw, term);
    ok &= oprf_nonzero(Dw);
    u32 d[8];
    {
        u32 Cw[8];
        u64 seed[8];
        load_c(Cw);
        load_seed(seed);
        oprf_composite_scalar(d, seed, idx, Cw, Dw);
    }
    {
        ge_pe rows[2];
        oprf_affine_table(rows, X, Y);
        oprf_walk(term, rows, d);
    }
    oprf_form_t(term);
#pragma unroll
    for (int i = 0; i < 8; i++) Dw[i] &= ok;
    return ok;
}

// stage (b) of the verifier for ONE of row i's two points: term = [d_i]C_i (second = zero) or [d_i]D_i (all-ones) extended with T.
// A lane per point: the row's two lanes both derive d_i (three compressions beside a walk) and neither holds anything for the other.
// load(k, w): the row's 32 bytes of blinded (k = 0) or evaluated (1); all-ones where the row is owned, neither of the two is the
// identity and this lane's decodes
template <typename Load, typename LoadSeed>
C25519_DEV u32 oprf_verifier_point_lane(ge_ext& term, const Load& load, const LoadSeed& load_seed, u32 idx, u32 owned, u32 second)
{
    u32 d[8], w[8], ok = owned;
    {
        u32 Cw[8], Dw[8];
        u64 seed[8];
        load(0u, Cw);
        load(1u, Dw);
        load_seed(seed);
        ok &= oprf_nonzero(Cw) & oprf_nonzero(Dw);
        oprf_composite_scalar(d, seed, idx, Cw, Dw);
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = (Cw[i] & ~second) | (Dw[i] & second);
    }
    fe X, Y;
    ok &= rist_decode(X, Y, w, 0u);
    ge_pe rows[2];
    oprf_affine_table(rows, X, Y);
    oprf_walk(term, rows, d);
    oprf_form_t(term);
    return ok;
}

// the sum of rows lo .. lo + count - 1 of `pts`; all-ones where every one of them is owned by request j.  Complete additions: the
// identity and repeated rows take the same code
C25519_DEV u32 oprf_sum_rows(ge_ext& M, const OprfPoints& pts, const u32* owner, size_t n, size_t lo, u32 count, u32 j)
{
    fe_set_u32(M.X, 0);
    fe_set_u32(M.Y, 1);
    fe_set_u32(M.Z, 1);
    fe_set_u32(M.T, 0);
    u32 good = 0xffffffffu;
#pragma unroll 1
    for (u32 k = 0; k < count; k++) {
        ge_ext Q;
        ge_pe q;
        oprf_load_point(Q, pts, n, lo + k);
        good &= group_eq_mask(owner[lo + k] >> 1, j >> 1) & group_eq_mask(owner[lo + k] & 1u, j & 1u);
        ge_to_pe(q, Q);
        ge_add_pe<true>(M, M, q);
    }
    return good;
}

// stage (c) of the server for one request: the proof c || s over M = sum [d_i]C_i (already summed: M extended with T), Z = [skS]M,
// t2 = [r]B, t3 = [r]M; returns all-ones where neither r nor skS is 0 mod L (and `good` says the rows are), zero words where not
template <typename ColT>
C25519_DEV u32 oprf_prove_lane(u32 (&proof)[16], const ge_ext& M, const u32 (&sks)[8], const u32 (&rw)[8], const OprfHead& h, u32 good,
                               const u32* __restrict__ g_wide, ColT* cols, int stride)
{
    u32 sk[8], r[8], Mw[8], Zw[8], t2w[8], t3w[8];
    oprf_scalar(sk, sks);
    oprf_scalar(r, rw);
    good &= sc_nonzero_mask(sk) & sc_nonzero_mask(r);
    rist_encode<true>(Mw, M);
    {
        ge_pe rows[2];
        ge_ext S;
        oprf_table(rows, M);
        oprf_walk(S, rows, sk);
        rist_encode<false>(Zw, S);
        oprf_walk(S, rows, r);
        rist_encode<false>(t3w, S);
    }
    {
        ge_ext S;
        wb_columns(cols, stride, r);                         // r + L when even: B has order L
        ge_base_mult_wide(S, g_wide, cols, stride);
        rist_encode<false>(t2w, S);
    }
    u32 c[8], s[8], t[8];
    oprf_challenge(c, h.pk, Mw, Zw, t2w, t3w);
    sc_mul(t, c, sk);
    sc_mod(t);
    sc_l_minus(t, t);                                        // L - c skS, in [1, L]
    sc_add(s, r, t);
    sc_mod(s);                                               // s = r - c skS mod L, canonical
#pragma unroll
    for (int i = 0; i < 8; i++) {
        proof[i] = c[i] & good;
        proof[8 + i] = s[i] & good;
    }
    return good;
}

// stage (c) of the verifier for one request: all-ones where c and s are canonical, pkS decodes and is not the identity, and the
// challenge recomputed from t2 = [s]B + [c]pkS, t3 = [s]M + [c]Z is c (M, Z extended with T)
template <typename ColT>
C25519_DEV u32 oprf_check_lane(const ge_ext& M, const ge_ext& Z, const u32 (&proof)[16], const OprfHead& h, u32 good,
                               const u32* __restrict__ g_wide, ColT* cols, int stride)
{
    u32 c[8], s[8], Mw[8], Zw[8], t2w[8], t3w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c[i] = proof[i];
        s[i] = proof[8 + i];
    }
    good &= strict_less(c, K_L) & strict_less(s, K_L);
    c[7] &= 0x0fffffffu;                                     // (a rejected proof walks as some scalar below 2^255)
    s[7] &= 0x0fffffffu;
    rist_encode<true>(Mw, M);
    rist_encode<true>(Zw, Z);
    ge_pe rows[2], q;
    ge_ext S, U;
    // t3 = [s]M + [c]Z
    oprf_table(rows, M);
    oprf_walk(U, rows, s);
    oprf_form_t(U);
    oprf_table(rows, Z);
    oprf_walk(S, rows, c);
    oprf_form_t(S);
    ge_to_pe(q, S);
    ge_add_pe<true>(U, U, q);
    rist_encode<true>(t3w, U);
    // t2 = [s]B + [c]pkS
    {
        fe X, Y;
        good &= rist_decode(X, Y, h.pk, 0u) & oprf_nonzero(h.pk);
        oprf_affine_ext(S, X, Y);
        oprf_table(rows, S);
        oprf_walk(S, rows, c);
        oprf_form_t(S);
        ge_to_pe(q, S);
    }
    wb_columns(cols, stride, s);                             // s + L when even: B has order L
    ge_base_mult_wide<true>(U, g_wide, cols, stride);
    ge_add_pe<true>(U, U, q);
    rist_encode<true>(t2w, U);
    u32 want[8], diff = 0;
    oprf_challenge(want, h.pk, Mw, Zw, t2w, t3w);
#pragma unroll
    for (int i = 0; i < 8; i++) diff |= want[i] ^ proof[i];
    return good & group_eq_mask(diff >> 1 | (diff & 1u), 0);
}

}  // namespace c25519
