// curve25519_amd/csrc/h2c25519.cuh -- what ONE lane does for the calls that hash messages to the groups (RFC 9380, RFC 9497;
// include/curve25519_amd.h states their rules):
//   c25519_ExpandMessageXmd_*      expand_message_xmd over SHA-512 (RFC 9380 section 5.3.1)
//   ed25519_MapToCurve_*           map_to_curve_elligator2_edwards25519(u) (6.8.2), encoded, no cofactor cleared
//   ed25519_HashToCurve_*          edwards25519_XMD:SHA-512_ELL2_RO_: two field elements, two maps, one addition, times 8
//   ed25519_EncodeToCurve_*        edwards25519_XMD:SHA-512_ELL2_NU_: one field element, one map, times 8
//   ristretto255_HashToGroup_*     64 expander bytes into ristretto255.cuh's rist_from_hash_lane (RFC 9380 appendix B)
//   ed25519_HashToScalar_*         64 expander bytes, little-endian, mod L (RFC 9497 section 4.1)
// engine_h2c.hip wraps these in its kernels; tests/host_emul/h2c.cpp drives the same functions on the CPU.
//
// The expander.  b_0 = H(Z_pad || msg || I2OSP(len_in_bytes, 2) || 0x00 || DST || I2OSP(dst_len, 1)), b_1 = H(b_0 || 0x01 || DST'),
// b_i = H((b_0 xor b_(i-1)) || i || DST').
//   * Z_pad is one whole block of zeros: its compression is the constant K_SHA512_ZPAD_MID (tools/gen_constants.py) and b_0 starts
//     from it.
//   * Everything behind the message is the same for every lane of a call, and so is where it starts (msg_size is uniform).  The host
//     lays it out ONCE per call (h2c_make_tail) as the big-endian 64-bit words the compression takes, already shifted by
//     msg_size % 8, with SHA-512's 0x80 and the bit length in place: H2cTail::w0 for b_0 from the word the message ends in, w1 for b_i
//     from the word behind the 64 bytes in registers (its first byte is left zero for i).  The kernels take the H2cTail BY VALUE:
//     the words are read with scalar loads from the kernel arguments, a call allocates and copies nothing, and a *_dev call is
//     one launch on the caller's stream.
//   * The message body is whole words through sha512_msg_word's aligned path; the word the message ends in is its last
//     msg_size % 8 bytes over w0[0]'s zeros.  Which words are message and which are tail is uniform: the block loop does not diverge.
// Messages are SECRET here (OPRF inputs, passwords), and so is everything derived from them: the expander's output, u, the points.
// Lengths and the DST are public.  No branch and no address depends on a secret (tests/host_emul/taint_h2c.cpp): the loops run
// on lengths, the map's CMOVs, its sgn0 fix-up and its exceptional case are masks, as in ristretto255.cuh, whose helpers it uses.
// Limb bounds (fe25519.cuh's contract; tools/fe_bounds.py replays h2c_fe_from_be48 and the map): every value named below is reduced
// unless a comment gives its beta.
#pragma once
#include "sha512.cuh"
#include "sc25519.cuh"
#include "ristretto255.cuh"

#include <stddef.h>

namespace c25519 {

constexpr int H2C_MAX_DST = 255;
constexpr int H2C_MAX_LEN = 255 * 64;                        // ell <= 255
// w0: at most 7 message bytes + 3 + 255 + 1 + 0x80 + 16 of length = 283 bytes, and up to 15 words of zeros to the block's end
constexpr int H2C_W0 = 52;
// w1: i + 255 + 1 + 0x80 + 16 = 274 bytes behind 64: three blocks less the eight words in registers
constexpr int H2C_W1 = 40;

struct H2cTail {
    u64 w0[H2C_W0];
    u64 w1[H2C_W1];
    u32 msg_words, msg_rem;                                  // msg_size / 8 and msg_size % 8
    u32 blocks0, blocks1;                                    // blocks of b_0 behind Z_pad; blocks of every b_i
    u32 len_in_bytes, ell;                                   // ExpandMessageXmd's output: bytes, and blocks b_1 .. b_ell
};

// byte k of a big-endian word array
inline void h2c_put_byte(u64* w, size_t k, unsigned byte) { w[k / 8] |= (u64)byte << (56 - 8 * (k % 8)); }

// the uniform part of a call, on the HOST (dst: dst_len bytes, 1 .. 255; len_in_bytes: 1 .. H2C_MAX_LEN; the callers check)
inline void h2c_make_tail(H2cTail& t, size_t msg_size, const unsigned char* dst, size_t dst_len, size_t len_in_bytes)
{
    for (int i = 0; i < H2C_W0; i++) t.w0[i] = 0;
    for (int i = 0; i < H2C_W1; i++) t.w1[i] = 0;
    t.msg_words = (u32)(msg_size / 8);
    t.msg_rem = (u32)(msg_size % 8);
    t.len_in_bytes = (u32)len_in_bytes;
    t.ell = (u32)((len_in_bytes + 63) / 64);
    // b_0 behind Z_pad: msg || l_i_b_str || 0 || DST || dst_len || 0x80 ... bit length
    const size_t total0 = msg_size + 4 + dst_len;
    t.blocks0 = (u32)((total0 + 17 + 127) / 128);
    size_t k = t.msg_rem;                                    // w0[0] is the word the message ends in
    h2c_put_byte(t.w0, k++, (unsigned)(len_in_bytes >> 8) & 0xffu);
    h2c_put_byte(t.w0, k++, (unsigned)len_in_bytes & 0xffu);
    k++;
    for (size_t j = 0; j < dst_len; j++) h2c_put_byte(t.w0, k++, dst[j]);
    h2c_put_byte(t.w0, k++, (unsigned)dst_len);
    h2c_put_byte(t.w0, k++, 0x80u);
    t.w0[16 * (size_t)t.blocks0 - 1 - t.msg_words] = (u64)(128 + total0) << 3;
    // b_i behind the 64 bytes in registers: i || DST || dst_len || 0x80 ... bit length
    const size_t total1 = 64 + 2 + dst_len;
    t.blocks1 = (u32)((total1 + 17 + 127) / 128);
    k = 1;
    for (size_t j = 0; j < dst_len; j++) h2c_put_byte(t.w1, k++, dst[j]);
    h2c_put_byte(t.w1, k++, (unsigned)dst_len);
    h2c_put_byte(t.w1, k++, 0x80u);
    t.w1[16 * (size_t)t.blocks1 - 1 - 8] = (u64)total1 << 3;
}

// b_0 of the lane's message (msg: 8 msg_words + msg_rem bytes, any alignment)
C25519_DEV void h2c_b0(u64 (&b0)[8], const uint8_t* msg, const H2cTail& t)
{
    u64 st[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = K_SHA512_ZPAD_MID[i];
    const size_t body = 8 * (size_t)t.msg_words;
    u64 last = 0;                                            // the message's last msg_rem bytes, at the top of their word
#pragma unroll
    for (u32 j = 0; j < 8; j++) last = (last << 8) | (j < t.msg_rem ? msg[body + j] : 0u);
#pragma unroll 1
    for (u32 blk = 0; blk < t.blocks0; blk++) {
#pragma unroll
        for (u32 j = 0; j < 16; j++) {
            const u32 g = 16 * blk + j;                      // word of the stream behind Z_pad
            u64 v;
            if (g < t.msg_words) v = sha512_msg_word(msg, body, g);
            else v = t.w0[g - t.msg_words] | (g == t.msg_words ? last : 0);
            w[j] = v;
        }
        sha512_compress(st, w);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) b0[i] = st[i];
}

// b_0 of a message whose first 32 bytes sit in registers as four stream words (pre: a key's bytes through sha512_words_from_le32)
// and whose other 8 (msg_words - 4) + msg_rem bytes are at `rest`, any alignment (not read where there are none): the tail is the
// one h2c_make_tail lays out for the whole length.  ECVRF's encode_to_curve(PK_string || alpha_string), vrf25519.cuh.
C25519_DEV void h2c_b0_pre4(u64 (&b0)[8], const u64 (&pre)[4], const uint8_t* rest, const H2cTail& t)
{
    u64 st[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = K_SHA512_ZPAD_MID[i];
    const size_t body = 8 * (size_t)(t.msg_words - 4);
    u64 last = 0;
#pragma unroll
    for (u32 j = 0; j < 8; j++) last = (last << 8) | (j < t.msg_rem ? rest[body + j] : 0u);
#pragma unroll 1
    for (u32 blk = 0; blk < t.blocks0; blk++) {
#pragma unroll
        for (u32 j = 0; j < 16; j++) {
            const u32 g = 16 * blk + j;
            u64 v;
            if (j < 4 && blk == 0) v = pre[j];
            else if (g < t.msg_words) v = sha512_msg_word(rest, body, g - 4);
            else v = t.w0[g - t.msg_words] | (g == t.msg_words ? last : 0);
            w[j] = v;
        }
        sha512_compress(st, w);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) b0[i] = st[i];
}

// b_i = H(in || i || DST'): in is b_0 for i = 1, b_0 xor b_(i-1) beyond
C25519_DEV void h2c_bi(u64 (&out)[8], const u64 (&in)[8], u32 i, const H2cTail& t)
{
    u64 st[8] = { 0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                  0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull };
    u64 w[16];
    const u64 first = t.w1[0] | ((u64)i << 56);
#pragma unroll 1
    for (u32 blk = 0; blk < t.blocks1; blk++) {
#pragma unroll
        for (u32 j = 0; j < 16; j++) {
            u64 v;
            if (j < 8) v = blk == 0 ? in[j] : t.w1[16 * blk + j - 8];
            else v = (j == 8 && blk == 0) ? first : t.w1[16 * blk + j - 8];
            w[j] = v;
        }
        sha512_compress(st, w);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = st[k];
}

// the first 64 (TWO = false) or 128 (true) bytes of expand_message_xmd as digest words: all the point and scalar calls read
template <bool TWO>
C25519_DEV void h2c_uniform(u64 (&b1)[8], u64 (&b2)[8], const uint8_t* msg, const H2cTail& t)
{
    u64 b0[8];
    h2c_b0(b0, msg, t);
    h2c_bi(b1, b0, 1, t);
    if (TWO) {
#pragma unroll
        for (int k = 0; k < 8; k++) b0[k] ^= b1[k];
        h2c_bi(b2, b0, 2, t);
    }
}

// c25519_ExpandMessageXmd for one element: out[0 .. len_in_bytes).  Rows are len_in_bytes apart from a 16-byte aligned base: whole
// words where that is a multiple of four (a uniform choice), bytes otherwise
C25519_DEV void h2c_expand_lane(uint8_t* out, const uint8_t* msg, const H2cTail& t)
{
    u64 b0[8], b[8], in[8];
    h2c_b0(b0, msg, t);
#pragma unroll
    for (int k = 0; k < 8; k++) in[k] = b0[k];
    const bool by_words = (t.len_in_bytes & 3u) == 0;
#pragma unroll 1
    for (u32 i = 1; i <= t.ell; i++) {
        h2c_bi(b, in, i, t);
        const u32 base = 64 * (i - 1);
#pragma unroll
        for (u32 k = 0; k < 8; k++) {
            if (by_words) {
                u32* o = reinterpret_cast<u32*>(out + base + 8 * k);
                if (base + 8 * k + 4 <= t.len_in_bytes) o[0] = __builtin_bswap32((u32)(b[k] >> 32));
                if (base + 8 * k + 8 <= t.len_in_bytes) o[1] = __builtin_bswap32((u32)b[k]);
            } else {
#pragma unroll
                for (u32 j = 0; j < 8; j++)
                    if (base + 8 * k + j < t.len_in_bytes) out[base + 8 * k + j] = (uint8_t)(b[k] >> (56 - 8 * j));
            }
        }
#pragma unroll
        for (int k = 0; k < 8; k++) in[k] = b0[k] ^ b[k];
    }
}

// 48 bytes, big-endian, mod p (hash_to_field's OS2IP with L = 48): d[0] is the most significant digest word, d[5] the least.  As
// twelve little-endian 32-bit words the low eight go through fe_from_words, which counts bit 255 as 19, and the top four (128
// bits: five limbs of at most 2^26 - 1, 2^25 - 1, ...) weigh 2^256 = 38: r = lo + 38 hi limb by limb, every limb below
// 39 * 2^w + 19 (beta 39: inside fe_carry32's beta < 2^6 and 32 bits), then one carry pass.  Reduced out.
C25519_DEV void h2c_fe_from_be48(fe& r, const u64 (&d)[6])
{
    u32 lo[8], hi[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        lo[2 * i] = (u32)d[5 - i];
        lo[2 * i + 1] = (u32)(d[5 - i] >> 32);
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        hi[2 * i] = (u32)d[1 - i];
        hi[2 * i + 1] = (u32)(d[1 - i] >> 32);
    }
#pragma unroll
    for (int i = 4; i < 8; i++) hi[i] = 0;
    fe a, b;
    fe_from_words(a, lo);
    fe_from_words(b, hi);                                    // limbs 5 .. 9 are zero
#pragma unroll
    for (int i = 0; i < 5; i++) a.v[i] += 38u * b.v[i];
    fe_carry32(r, a);
}

// all-ones iff a == b mod p; a any beta <= 3, b reduced
C25519_DEV u32 h2c_fe_eq(const fe& a, const fe& b)
{
    fe t;
    fe_sub(t, a, b);                                         // beta a + 2
    return rist_is_zero(t);
}

// map_to_curve_elligator2_edwards25519(u), RFC 9380 section 6.8.2, by appendix G.2.1 (Elligator 2 to curve25519, one x^((p-5)/8)
// chain) and G.2.2 (the rational map), in the RFC's operation order: P in extended coordinates, u reduced.  No cofactor cleared.
// e1 .. e4 and the exceptional case are masks.  u = 0 (the Montgomery point (0, 0)) gives the identity; x = -1 would too and has
// no u (tools/gen_constants.py asserts both).
C25519_DEV void h2c_map(ge_ext& P, const fe& u)
{
    fe J, tv1, tv2, tv3, xd, gxd, gx1, gx2, y11, y12, y1, y21, y22, y2, x2n, xn, y, t, one;
    fe_set_u32(J, 486662u);
    fe_set_u32(one, 1);
    fe_sqr(tv1, u);
    fe_add(t, tv1, tv1);                                     // beta 2
    fe_carry32(tv1, t);                                      // tv1 = 2 u^2
    xd = tv1;
    xd.v[0] += 1;                                            // xd = tv1 + 1, never zero: -1 / 2 is no square
    fe_sqr(tv2, xd);
    fe_mul(gxd, tv2, xd);                                    // gxd = xd^3
    fe_mul(gx1, tv1, J);
    fe_mul(gx1, gx1, fe_const(K_H2C_NEG_J));                 // x1n J tv1
    fe_add(gx1, gx1, tv2);                                   // beta 2
    fe_mul(gx1, gx1, fe_const(K_H2C_NEG_J));                 // gx1 = x1n^3 + J x1n^2 xd + x1n xd^2
    fe_sqr(tv3, gxd);
    fe_sqr(tv2, tv3);                                        // gxd^4
    fe_mul(tv3, tv3, gxd);
    fe_mul(tv3, tv3, gx1);                                   // gx1 gxd^3
    fe_mul(tv2, tv2, tv3);                                   // gx1 gxd^7
    fe_pow2523(y11, tv2);
    fe_mul(y11, y11, tv3);                                   // y11 = gx1 gxd^3 (gx1 gxd^7)^((p-5)/8)
    fe_mul(y12, y11, fe_const(K_SQRTM1));
    fe_sqr(t, y11);
    fe_mul(t, t, gxd);
    const u32 e1 = h2c_fe_eq(t, gx1);
    fe_select(y1, e1, y11, y12);
    fe_mul(x2n, tv1, fe_const(K_H2C_NEG_J));                 // x2n = x1n tv1
    fe_mul(y21, y11, u);
    fe_mul(y21, y21, fe_const(K_H2C_C2));
    fe_mul(y22, y21, fe_const(K_SQRTM1));
    fe_mul(gx2, gx1, tv1);
    fe_sqr(t, y21);
    fe_mul(t, t, gxd);
    const u32 e2 = h2c_fe_eq(t, gx2);
    fe_select(y2, e2, y21, y22);
    fe_sqr(t, y1);
    fe_mul(t, t, gxd);
    const u32 e3 = h2c_fe_eq(t, gx1);                        // gx1 is a square: (x1, y1), with sgn0(y) = 1; else (x2, y2), sgn0(y) = 0
    fe_select(xn, e3, fe_const(K_H2C_NEG_J), x2n);
    fe_select(y, e3, y1, y2);
    const u32 e4 = rist_is_negative(y);
    rist_cneg(y, y, e3 ^ e4);
    // (xMn, xMd, yMn, yMd) = (xn, xd, y, 1) -> Edwards (xn / xd, yn / yd)
    fe en, ed, yn, yd;
    fe_mul(en, xn, fe_const(K_H2C_SQRT_M486664));
    fe_mul(ed, xd, y);
    fe_sub(t, xn, xd);                                       // beta 3
    fe_carry32(yn, t);
    fe_add(t, xn, xd);                                       // beta 2
    fe_carry32(yd, t);
    fe_mul(t, ed, yd);
    const u32 e = rist_is_zero(t);                           // a denominator vanishes: the identity
    fe zero;
    fe_set_u32(zero, 0);
    fe_select(en, e, zero, en);
    fe_select(ed, e, one, ed);
    fe_select(yn, e, one, yn);
    fe_select(yd, e, one, yd);
    fe_mul(P.X, en, yd);
    fe_mul(P.Y, yn, ed);
    fe_mul(P.Z, ed, yd);
    fe_mul(P.T, en, yn);
}

// the 32-byte Ed25519 encoding of S, T not read: the lane's own inversion by division steps (engine_h2c.hip says why it is not shared)
C25519_DEV void h2c_encode(u32 (&out)[8], const ge_ext& S)
{
    u32 xw[8], yw[8];
    ge_to_affine_words(xw, yw, S);
    ge_pack(out, xw, yw);
}

// ed25519_MapToCurve for one element: u is the 32 bytes with bit 255 masked, mod p
C25519_DEV void h2c_map_lane(u32 (&out)[8], const u32 (&uw)[8])
{
    fe u;
    ge_ext P;
    rist_hash_half(u, uw);
    h2c_map(P, u);
    h2c_encode(out, P);
}

// ed25519_HashToCurve (COUNT = 2) / ed25519_EncodeToCurve (COUNT = 1) for one element: hash_to_field(msg, COUNT), COUNT maps, their
// sum, three doublings, one inversion.  Projective throughout.
template <int COUNT>
C25519_DEV void h2c_to_curve_lane(u32 (&out)[8], const uint8_t* msg, const H2cTail& t)
{
    fe u0, u1;
    {
        u64 b1[8], b2[8], d[6];
        h2c_uniform<COUNT == 2>(b1, b2, msg, t);
#pragma unroll
        for (int k = 0; k < 6; k++) d[k] = b1[k];
        h2c_fe_from_be48(u0, d);
        if (COUNT == 2) {
#pragma unroll
            for (int k = 0; k < 6; k++) d[k] = k < 2 ? b1[6 + k] : b2[k - 2];
            h2c_fe_from_be48(u1, d);
        }
    }
    ge_ext S;
    ge_pe q;
    // the second element first, parked in precomputed form; the digests are dead before the maps start.  (The two maps as one
    // rolled loop keep the map's five constants in registers across it, 50 of them, and spilled 33 at two waves per SIMD.)
    if (COUNT == 2) {
        h2c_map(S, u1);
        ge_to_pe(q, S);
    }
    h2c_map(S, u0);
    if (COUNT == 2) ge_add_pe<false>(S, S, q);
    ge_double<false>(S);
    ge_double<false>(S);
    ge_double<false>(S);
    h2c_encode(out, S);
}

// ristretto255_HashToGroup for one element
C25519_DEV void h2c_to_group_lane(u32 (&out)[8], const uint8_t* msg, const H2cTail& t)
{
    u64 b1[8], b2[8];
    h2c_uniform<false>(b1, b2, msg, t);
    u32 h[16], lo[8], hi[8];
    sha512_digest_le_words(h, b1);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        lo[i] = h[i];
        hi[i] = h[8 + i];
    }
    rist_from_hash_lane(out, lo, hi);
}

// ed25519_HashToScalar for one element: canonical out
C25519_DEV void h2c_to_scalar_lane(u32 (&out)[8], const uint8_t* msg, const H2cTail& t)
{
    u64 b1[8], b2[8];
    h2c_uniform<false>(b1, b2, msg, t);
    u32 h[16];
    sha512_digest_le_words(h, b1);
    sc_reduce512(out, h);
}

}  // namespace c25519
