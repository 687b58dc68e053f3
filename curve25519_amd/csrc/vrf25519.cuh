// curve25519_amd/csrc/vrf25519.cuh -- what ONE lane does for ECVRF-EDWARDS25519-SHA512-ELL2 (RFC 9381, suite string 0x04;
// include/curve25519_amd.h states the calls' rules):
//   ed25519_VRF_Prove_*         pi = Gamma_string || c || s from the 64-byte private key and alpha (sections 5.1, 5.4.2.2, 5.4.3)
//   ed25519_VRF_Verify_*        the verdict and beta from the key, pi and alpha (5.3 with validate_key = TRUE, 5.4.5)
//   ed25519_VRF_ProofToHash_*   beta from pi alone (5.2, 5.4.4)
// engine_vrf.hip wraps these in its kernels; tests/host_emul/vrf.cpp drives the same functions on the CPU.
//
// Nothing new in the field or the group: the lane strings together the pieces the other calls have and keeps what is secret in
// registers from the seed to the proof.
//   * H = encode_to_curve(PK_string || alpha_string) under the DST "ECVRF_" || "edwards25519_XMD:SHA-512_ELL2_NU_" || 0x04: the
//     expander's b_0 takes the key's 32 bytes from registers (h2c_b0_pre4) and alpha from memory, the tail is h2c_make_tail's for
//     32 + alpha_size bytes; then one map and three doublings (h2c25519.cuh).
//   * [x]H, [k]H, [s]H, [c]Y, [c]Gamma: ed_group.cuh's masked walk at window width 2 (the width that keeps two rows of table and a
//     walk in 256 registers), its table built ONCE per point -- x and k walk H's in turn -- and its length a template parameter:
//     129 digits for a scalar below 2^255, 65 for the 128 bits of c.  The recoding is the group calls': one addition of
//     C = sum 2^(2 i + 1), whose two-bit fields are then d_i + 2 (vrf_recode says when the sum fits).
//   * [k]B and [s]B: the wide comb (ge_base_mult_wide), as ed25519_ScalarMultBase walks it.
//   * Encodings: every point a hash needs goes through ONE inversion a batch (vrf_invert_all, Montgomery's trick in the lane): H
//     alone in Prove (k is a hash of H_string), then Gamma, U, V together; H, U, V and [8]Gamma together in Verify.
//   * The short hashes -- 64 bytes for k, 163 for c, 35 for beta -- are laid out with their padding at compile time (vrf_put32).
// Secret in Prove: the seed, SHA-512(seed), x, k and what s is computed from.  Public: Y, alpha, H, Gamma, U, V, c, s.  No branch
// and no address derives from a secret but the comb's row fetch for [k]B (wb_load_pa_signed, as in signing), and no secret is
// stored (tests/host_emul/taint_vrf.cpp).  Verify and ProofToHash handle public data only; they are written with the same masks
// because a wave gains nothing from per-lane branches.
// Limb bounds (fe25519.cuh's contract): every value named below is reduced unless a comment gives its beta.
#pragma once
#include "ed_group.cuh"
#include "h2c25519.cuh"
#include "strict25519.cuh"

namespace c25519 {

constexpr int VRF_PROOF_WORDS = 20, VRF_BETA_WORDS = 16;    // ed25519_vrf_proof_size / ed25519_vrf_output_size in 32-bit words
constexpr int VRF_DIGITS_FULL = 129, VRF_DIGITS_C = 65;      // two-bit signed digits of a scalar below 2^255 / below 2^128
constexpr int VRF_DST_LEN = 40;
constexpr unsigned char VRF_SUITE = 0x04;

// "ECVRF_" || "edwards25519_XMD:SHA-512_ELL2_NU_" || suite_string, on the HOST
inline void vrf_dst(unsigned char (&dst)[VRF_DST_LEN])
{
    const char s[] = "ECVRF_edwards25519_XMD:SHA-512_ELL2_NU_";
    static_assert(sizeof s == VRF_DST_LEN, "39 characters and the suite byte");
    for (int i = 0; i < VRF_DST_LEN - 1; i++) dst[i] = (unsigned char)s[i];
    dst[VRF_DST_LEN - 1] = VRF_SUITE;
}

// the uniform part of a call's encode_to_curve, on the HOST: the message is the key's 32 bytes and alpha_size more
inline void vrf_make_tail(H2cTail& t, size_t alpha_size)
{
    unsigned char dst[VRF_DST_LEN];
    vrf_dst(dst);
    h2c_make_tail(t, 32 + alpha_size, dst, VRF_DST_LEN, 48);
}

// H = encode_to_curve(yw's 32 bytes || alpha), projective: T is not formed
C25519_DEV void vrf_hash_point(ge_ext& H, const u32 (&yw)[8], const uint8_t* alpha, const H2cTail& t)
{
    fe u;
    {
        u64 pre[4], b0[8], b1[8], d[6];
        sha512_words_from_le32(pre, yw);
        h2c_b0_pre4(b0, pre, alpha, t);
        h2c_bi(b1, b0, 1, t);
#pragma unroll
        for (int k = 0; k < 6; k++) d[k] = b1[k];
        h2c_fe_from_be48(u, d);
    }
    h2c_map(H, u);
    ge_double<false>(H);
    ge_double<false>(H);
    ge_double<false>(H);
}

// RFC 8032's decoding: all-ones iff the bytes decode and are the canonical encoding (ed25519_ClassifyKey's DECODES and CANONICAL:
// y < p, and not x = 0 under a set sign bit); X, Y: the point, or what the decoder left
C25519_DEV u32 vrf_decode(fe& X, fe& Y, const u32 (&w)[8])
{
    const u32 decodes = ed_zip215_decode(X, Y, w, 0u);
    u32 yw[8], xw[8], x_bits = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) yw[i] = w[i];
    yw[7] &= 0x7fffffffu;
    fe_to_words(xw, X);
#pragma unroll
    for (int i = 0; i < 8; i++) x_bits |= xw[i];
    const u32 zero_x_signed = group_eq_mask(x_bits >> 1 | (x_bits & 1u), 0) & (0u - (w[7] >> 31));
    return decodes & strict_less(yw, K_P) & ~zero_x_signed;
}

// (x, y) -> (-x, y) as an extended point with Z = 1 (negate: all-ones) or the point itself (zero)
C25519_DEV void vrf_affine_ext(ge_ext& P, const fe& X, const fe& Y, u32 negate)
{
    fe t;
    fe_neg(t, X);
    fe_carry32(t, t);
    fe_select(P.X, negate, t, X);
    P.Y = Y;
    fe_set_u32(P.Z, 1);
    fe_mul(P.T, P.X, Y);
}

// rows 1P and 2P of a walk's table; P with T
C25519_DEV void vrf_table(ge_pe (&rows)[2], const ge_ext& P)
{
    ge_ext Q;
    ge_to_pe(rows[0], P);
    ge_add_pe<true>(Q, P, rows[0]);
    ge_to_pe(rows[1], Q);
}

// C = sum_i 2^(2 i + 1) over N digits
template <int N>
C25519_DEV constexpr GroupOffset<2> vrf_offset()
{
    GroupOffset<2> c{};
    for (int i = 0; i < N; i++) c.w[(2 * i + 1) >> 5] |= 1u << ((2 * i + 1) & 31);
    return c;
}

// t = (e + C) << (288 - 2 N): the top digit's field in the top two bits of word 8, as group_next_field<2> takes them.  e + C fits
// 2 N bits for e < 4^N / 3 (C = 2 (4^N - 1) / 3): below 2^255 at N = 129, below 2^128 at N = 65.
template <int N>
C25519_DEV void vrf_recode(u32 (&t)[9], const u32 (&e)[8])
{
    constexpr GroupOffset<2> C = vrf_offset<N>();
    constexpr int S = 288 - 2 * N, WS = S / 32, BS = S % 32;
    static_assert(N >= 1 && 2 * N <= 288 - 30, "two words of headroom for the sum");
    u32 s[9];
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (u64)e[i] + C.w[i];
        s[i] = (u32)c;
        c >>= 32;
    }
    s[8] = (u32)c + C.w[8];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const u32 hi = i - WS >= 0 ? s[i - WS >= 0 ? i - WS : 0] : 0u;
        const u32 lo = i - WS - 1 >= 0 ? s[i - WS - 1 >= 0 ? i - WS - 1 : 0] : 0u;
        t[i] = BS ? (hi << BS) | (lo >> ((32 - BS) & 31)) : hi;
    }
}

// the affine precomputed form of (x, y)
C25519_DEV void vrf_to_pa(ge_pa& A, const fe& x, const fe& y)
{
    fe t;
    fe_add(t, y, x);  fe_carry32(A.ypx, t);
    fe_sub(t, y, x);  fe_carry32(A.ymx, t);
    fe_mul(t, x, y);
    fe_mul(A.t2d, t, fe_const(K_2D));
}

// q = d * P for the field f = d + 2 over AFFINE rows P and 2P: group_select<2> without the fourth field (the neutral row is
// (1, 1, 0)), for a table that could share an inversion (H's, below): 60 limbs instead of 80 and an addition of 7 products
C25519_DEV void vrf_select(ge_pa& q, const ge_pa (&rows)[2], u32 f)
{
    const u32 neg = ((f >> 1) & 1u) - 1u;                    // all-ones: f < 2, a negative digit
    const u32 mag = ((f - 2u) ^ neg) - neg;                  // |d| in [0, 2]
    const u32 zero = group_eq_mask(mag, 0);
    fe ypx, ymx, t2d, n;
    fe_set_u32(ypx, 1u & zero);
    fe_set_u32(ymx, 1u & zero);
    fe_set_u32(t2d, 0);
#pragma unroll
    for (u32 j = 0; j < 2; j++) {
        const u32 m = group_eq_mask(mag, j + 1);
#pragma unroll
        for (int i = 0; i < 10; i++) {
            ypx.v[i] |= rows[j].ypx.v[i] & m;
            ymx.v[i] |= rows[j].ymx.v[i] & m;
            t2d.v[i] |= rows[j].t2d.v[i] & m;
        }
    }
    fe_select(q.ypx, neg, ymx, ypx);
    fe_select(q.ymx, neg, ypx, ymx);
    fe_neg(n, t2d);                                          // 2p - 2dxy: beta 2, fine as the second factor of a product
    fe_select(q.t2d, neg, n, t2d);
}
C25519_DEV void vrf_select(ge_pe& q, const ge_pe (&rows)[2], u32 f) { group_select<2>(q, rows, f); }
C25519_DEV void vrf_add(ge_ext& S, const ge_pa& q) { ge_add_pa<false>(S, q); }
C25519_DEV void vrf_add(ge_ext& S, const ge_pe& q) { ge_add_pe<false>(S, S, q); }

// S = [e]P over P's table (ge_pa or ge_pe rows), e below vrf_recode<N>'s bound; T of the result is not formed.  ed_group_walk<2>
// at N digits.
template <int N, typename Row>
C25519_DEV void vrf_walk(ge_ext& S, const Row (&rows)[2], const u32 (&e)[8])
{
    u32 t[9];
    vrf_recode<N>(t, e);
    fe_set_u32(S.X, 0);
    fe_set_u32(S.Y, 1);
    fe_set_u32(S.Z, 1);
    fe_set_u32(S.T, 0);
#pragma unroll 1
    for (int i = 0; i < N; i++) {
        ge_double<false>(S);
        ge_double<true>(S);
        Row q;
        vrf_select(q, rows, group_next_field<2>(t));
        vrf_add(S, q);
    }
}

// the same point with T: (X Z, Y Z, Z^2, X Y)
C25519_DEV void vrf_form_t(ge_ext& S)
{
    fe_mul(S.T, S.X, S.Y);
    fe_mul(S.X, S.X, S.Z);
    fe_mul(S.Y, S.Y, S.Z);
    fe_sqr(S.Z, S.Z);
}

// zi[j] = 1 / z[j] by one inversion (a zero among them, which no curve point has, zeroes them all)
template <int K>
C25519_DEV void vrf_invert_all(fe (&zi)[K], const fe (&z)[K])
{
    fe pre[K], inv;
    pre[0] = z[0];
#pragma unroll
    for (int j = 1; j < K; j++) fe_mul(pre[j], pre[j - 1], z[j]);
    fe_invert(inv, pre[K - 1]);
#pragma unroll
    for (int j = K - 1; j > 0; j--) {
        fe_mul(zi[j], inv, pre[j - 1]);
        fe_mul(inv, inv, z[j]);
    }
    zi[0] = inv;
}

// enc(X / Z, Y / Z) given 1 / Z
C25519_DEV void vrf_encode(u32 (&out)[8], const ge_ext& S, const fe& zinv)
{
    fe t;
    u32 xw[8], yw[8];
    fe_mul(t, S.X, zinv);  fe_to_words(xw, t);
    fe_mul(t, S.Y, zinv);  fe_to_words(yw, t);
    ge_pack(out, xw, yw);
}

// H = encode_to_curve(yw's 32 bytes || alpha) as H_string and as the affine rows H, 2H of its walks: one inversion for both
C25519_DEV void vrf_hash_rows(ge_pa (&rows)[2], u32 (&Hw)[8], const u32 (&yw)[8], const uint8_t* alpha, const H2cTail& t)
{
    ge_ext H, D;
    vrf_hash_point(H, yw, alpha, t);
    D = H;
    ge_double<false>(D);
    fe z[2] = { H.Z, D.Z }, zi[2], x, y;
    vrf_invert_all<2>(zi, z);
    u32 xw[8], hyw[8];
    fe_mul(x, H.X, zi[0]);
    fe_mul(y, H.Y, zi[0]);
    fe_to_words(xw, x);
    fe_to_words(hyw, y);
    ge_pack(Hw, xw, hyw);
    vrf_to_pa(rows[0], x, y);
    fe_mul(x, D.X, zi[1]);
    fe_mul(y, D.Y, zi[1]);
    vrf_to_pa(rows[1], x, y);
}

// the 32 bytes v (little-endian words as they sit in memory) at byte OFF of the big-endian word array w, OFF even
template <int OFF>
C25519_DEV void vrf_put32(u64* w, const u32 (&v)[8])
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

// c = the first 16 bytes of SHA-512(suite || 0x02 || Y || H || Gamma || U || V || 0x00): 163 bytes, two blocks (5.4.3)
C25519_DEV void vrf_challenge(u32 (&c)[4], const u32 (&Yw)[8], const u32 (&Hw)[8], const u32 (&Gw)[8], const u32 (&Uw)[8], const u32 (&Vw)[8])
{
    u64 w[32];
#pragma unroll
    for (int i = 0; i < 32; i++) w[i] = 0;
    w[0] = ((u64)VRF_SUITE << 56) | ((u64)0x02 << 48);
    vrf_put32<2>(w, Yw);
    vrf_put32<34>(w, Hw);
    vrf_put32<66>(w, Gw);
    vrf_put32<98>(w, Uw);
    vrf_put32<130>(w, Vw);
    w[163 / 8] |= (u64)0x80 << (56 - 8 * (163 % 8));         // byte 162 is the trailing 0x00
    w[31] = (u64)163 << 3;
    u64 st[8] = { 0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                  0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull };
    u64 blk[16];
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = w[i];
    sha512_compress(st, blk);
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = w[16 + i];
    sha512_compress(st, blk);
    c[0] = __builtin_bswap32((u32)(st[0] >> 32));
    c[1] = __builtin_bswap32((u32)st[0]);
    c[2] = __builtin_bswap32((u32)(st[1] >> 32));
    c[3] = __builtin_bswap32((u32)st[1]);
}

// beta = SHA-512(suite || 0x03 || enc([8]Gamma) || 0x00): 35 bytes, one block (5.2)
C25519_DEV void vrf_beta(u32 (&beta)[VRF_BETA_WORDS], const u32 (&G8w)[8])
{
    u64 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = 0;
    w[0] = ((u64)VRF_SUITE << 56) | ((u64)0x03 << 48);
    vrf_put32<2>(w, G8w);
    w[35 / 8] |= (u64)0x80 << (56 - 8 * (35 % 8));
    w[15] = (u64)35 << 3;
    u64 st[8] = { 0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                  0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull };
    sha512_compress(st, w);
    sha512_digest_le_words(beta, st);
}

// the fields of pi: Gamma's bytes, c as a 256-bit scalar, s
C25519_DEV void vrf_split_proof(u32 (&Gw)[8], u32 (&c)[8], u32 (&s)[8], const u32 (&pi)[VRF_PROOF_WORDS])
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        Gw[i] = pi[i];
        c[i] = i < 4 ? pi[8 + i] : 0u;
        s[i] = pi[12 + i];
    }
}

// ed25519_VRF_Prove for one element.  key: the element's 64-byte private key behind two calls, seed(w) and pk(w) (the second half
// as given: not recomputed, not checked) -- the lane reads each half where it needs it and again at the end (x is derived twice,
// one compression) instead of carrying sixteen words through the walks; alpha: this element's alpha_size bytes; cols: the lane's
// parked comb columns, `stride` elements apart
template <typename Key, typename ColT>
C25519_DEV void vrf_prove_lane(u32 (&pi)[VRF_PROOF_WORDS], const Key& key, const uint8_t* alpha, const H2cTail& t,
                               const u32* __restrict__ g_wide, ColT* cols, int stride)
{
    u32 k[8], Hw[8], Gw[8], Uw[8], Vw[8];
    ge_pa rows[2];
    {
        u32 yw[8];
        key.pk(yw);
        vrf_hash_rows(rows, Hw, yw, alpha, t);
    }
    {
        ge_ext G, U, V;
        {
            u32 seed[8], x[8], le[16];
            u64 pre[8], b_words[4], dg[8];
            key.seed(seed);
            ed_expand_seed(x, b_words, seed);                // x = SHA-512(seed)[0 .. 31] clamped
#pragma unroll
            for (int i = 0; i < 4; i++) pre[i] = b_words[i];
            sha512_words_from_le32(pre + 4, Hw);
            sha512_prefixed<8>(dg, pre, nullptr, 0);         // k = SHA-512(SHA-512(seed)[32 .. 63] || H_string) mod L (5.4.2.2)
            sha512_digest_le_words(le, dg);
            sc_reduce512(k, le);
            sc_mod(k);
            vrf_walk<VRF_DIGITS_FULL>(G, rows, x);
        }
        vrf_walk<VRF_DIGITS_FULL>(V, rows, k);
        wb_columns(cols, stride, k);                         // k + L when even: B has order L
        ge_base_mult_wide(U, g_wide, cols, stride);
        fe z[3] = { G.Z, U.Z, V.Z }, zi[3];
        vrf_invert_all<3>(zi, z);
        vrf_encode(Gw, G, zi[0]);
        vrf_encode(Uw, U, zi[1]);
        vrf_encode(Vw, V, zi[2]);
    }
    u32 c[8], s[8];
    {
        u32 yw[8], c4[4];
        key.pk(yw);
        vrf_challenge(c4, yw, Hw, Gw, Uw, Vw);
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = i < 4 ? c4[i] : 0u;
    }
    {
        u32 seed[8], x[8];
        u64 b_words[4];
        key.seed(seed);
        ed_expand_seed(x, b_words, seed);
        sc_mul(s, c, x);
    }
    sc_add(s, s, k);
    sc_mod(s);                                               // s = k + c x mod L, canonical
#pragma unroll
    for (int i = 0; i < 8; i++) {
        pi[i] = Gw[i];
        if (i < 4) pi[8 + i] = c[i];
        pi[12 + i] = s[i];
    }
}

// ed25519_VRF_ProofToHash for one element: all-ones iff pi decodes (Gamma canonically, s < L); beta is zeroed where it does not
C25519_DEV u32 vrf_proof_to_hash_lane(u32 (&beta)[VRF_BETA_WORDS], const u32 (&pi)[VRF_PROOF_WORDS])
{
    u32 Gw[8], c[8], s[8];
    vrf_split_proof(Gw, c, s, pi);
    fe X, Y;
    const u32 ok = vrf_decode(X, Y, Gw) & strict_less(s, K_L);
    ge_ext G;
    G.X = X;
    G.Y = Y;
    fe_set_u32(G.Z, 1);
    ge_double<false>(G);
    ge_double<false>(G);
    ge_double<false>(G);
    fe zi;
    fe_invert(zi, G.Z);
    vrf_encode(Gw, G, zi);
    vrf_beta(beta, Gw);
#pragma unroll
    for (int i = 0; i < VRF_BETA_WORDS; i++) beta[i] &= ok;
    return ok;
}

// ed25519_VRF_Verify for one element: all-ones iff the key decodes canonically and is not of small order, pi decodes, and the 16
// bytes recomputed from (Y, H, Gamma, U = [s]B - [c]Y, V = [s]H - [c]Gamma) are pi's c; beta is zeroed where not
template <typename ColT>
C25519_DEV u32 vrf_verify_lane(u32 (&beta)[VRF_BETA_WORDS], const u32 (&pkw)[8], const u32 (&pi)[VRF_PROOF_WORDS], const uint8_t* alpha,
                               const H2cTail& t, const u32* __restrict__ g_wide, ColT* cols, int stride)
{
    u32 Gw[8], c[8], s[8];
    vrf_split_proof(Gw, c, s, pi);
    fe X, Y;
    u32 ok = strict_less(s, K_L) & ~strict_small_y(pkw);
    ge_ext P, U, V, G8;
    ge_pe rows[2], q;
    u32 Hw[8], Uw[8], Vw[8], G8w[8];
    // V = [s]H + [c](-Gamma); an s that is not below L (the row is rejected) walks as its low 255 bits
    {
        ge_pa hrows[2];
        u32 e[8];
        vrf_hash_rows(hrows, Hw, pkw, alpha, t);
#pragma unroll
        for (int i = 0; i < 8; i++) e[i] = s[i];
        e[7] &= 0x7fffffffu;
        vrf_walk<VRF_DIGITS_FULL>(V, hrows, e);
        vrf_form_t(V);
    }
    ok &= vrf_decode(X, Y, Gw);
    vrf_affine_ext(G8, X, Y, 0u);                            // [8]Gamma
    ge_double<false>(G8);
    ge_double<false>(G8);
    ge_double<false>(G8);
    vrf_affine_ext(P, X, Y, 0xffffffffu);
    vrf_table(rows, P);
    vrf_walk<VRF_DIGITS_C>(P, rows, c);
    vrf_form_t(P);
    ge_to_pe(q, P);
    ge_add_pe<false>(V, V, q);
    // U = [s]B + [c](-Y)
    ok &= vrf_decode(X, Y, pkw);
    vrf_affine_ext(P, X, Y, 0xffffffffu);
    vrf_table(rows, P);
    vrf_walk<VRF_DIGITS_C>(P, rows, c);
    vrf_form_t(P);
    ge_to_pe(q, P);
    wb_columns(cols, stride, s);                             // s + L when even: B has order L
    ge_base_mult_wide<true>(U, g_wide, cols, stride);
    ge_add_pe<false>(U, U, q);
    {
        fe z[3] = { U.Z, V.Z, G8.Z }, zi[3];
        vrf_invert_all<3>(zi, z);
        vrf_encode(Uw, U, zi[0]);
        vrf_encode(Vw, V, zi[1]);
        vrf_encode(G8w, G8, zi[2]);
    }
    u32 c4[4], diff = 0;
    vrf_challenge(c4, pkw, Hw, Gw, Uw, Vw);
#pragma unroll
    for (int i = 0; i < 4; i++) diff |= c4[i] ^ c[i];
    ok &= group_eq_mask(diff >> 1 | (diff & 1u), 0);
    vrf_beta(beta, G8w);
#pragma unroll
    for (int i = 0; i < VRF_BETA_WORDS; i++) beta[i] &= ok;
    return ok;
}

}  // namespace c25519
