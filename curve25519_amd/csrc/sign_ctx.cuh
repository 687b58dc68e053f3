// curve25519_amd/csrc/sign_ctx.cuh -- ed25519_SignMessage against MANY signer contexts in one call (ed25519_Sign_Init_*,
// ed25519_SignMessage_indexed_*): element i is signed under context ctx_index[i] of the call's n_ctx 128-byte records
//   words  0..7   a       H(seed)[0..31] clamped (ecp_TrimSecretKey)
//   words  8..15  prefix  H(seed)[32..63]
//   words 16..23  pk      privKey[32..63] as given (the reference hashes the given half: ed25519_sign.c:406)
//   words 24..31  zero (ignored)
// so the H(seed) compression of ed25519_SignMessage (ed25519_sign.c:384-389) is done once per key, by Sign_Init, instead of
// once per signature.  The three signing forms of the engine each have their counterpart here -- one lane per element
// (k_ed25519_sign_indexed_mult / _finish around the shared inversion), four lanes per element (quad::sign_ctx_element), one
// element per wave (coop::sign_ctx_one) -- the same steps as ed_sign_nonce / ed_sign_s with the key taken from the context.
// In a header of its own so that tests/host_emul compiles it too.
//
// The index is public data (which key signs), so its gather and bounds check take no constant-time care; the secret only enters
// the hashes and the comb walk, as in every other signature.  An index >= n_ctx reads nothing and gives 64 zero bytes.
#pragma once
#include "lanes.cuh"
#include "coop_ops.cuh"
#include "quad25519.cuh"

namespace c25519 {

constexpr size_t SCTX_BYTES = 128, SCTX_WORDS = SCTX_BYTES / 4;
constexpr size_t SCTX_A = 0, SCTX_PREFIX = 1, SCTX_PK = 2;          // 32-byte records of a context

// element i's context, or null when its index is out of range
C25519_DEV const u32* sign_ctx_of(const u32* ctxs, size_t n_ctx, const u32* ctx_index, size_t i)
{
    const u32 k = ctx_index[i];
    return k < n_ctx ? ctxs + (size_t)k * SCTX_WORDS : nullptr;
}

// ed25519_Sign_Init for key e: ctx e = a || prefix || pk || 0 from priv e = seed || pk
C25519_DEV void sign_ctx_init_lane(void* ctxs, const void* priv, size_t e)
{
    u32 seed[8], pkw[8], a[8], pw[8];
    const u32 zero[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    u64 b_words[4];
    load32(seed, priv, 2 * e);
    load32(pkw, priv, 2 * e + 1);
    ed_expand_seed(a, b_words, seed);
#pragma unroll
    for (int i = 0; i < 4; i++) {                          // big-endian stream words -> the digest's bytes 32..63
        pw[2 * i] = __builtin_bswap32((u32)(b_words[i] >> 32));
        pw[2 * i + 1] = __builtin_bswap32((u32)b_words[i]);
    }
    store32(ctxs, 4 * e + SCTX_A, a);
    store32(ctxs, 4 * e + SCTX_PREFIX, pw);
    store32(ctxs, 4 * e + SCTX_PK, pkw);
    store32(ctxs, 4 * e + 3, zero);
}

// r = H(prefix || m) mod L, canonical, with the context's prefix   (ed25519_sign.c:392-397)
template <typename Sha = ShaPlain>
C25519_DEV void sign_ctx_r(u32 (&r)[8], const u32* ctx, const uint8_t* msg, size_t len, const Sha& sha = Sha())
{
    u32 pw[8];
    u64 b_words[4];
    load32(pw, ctx, SCTX_PREFIX);
    sha512_words_from_le32(b_words, pw);
    ed_sign_r(r, b_words, msg, len, sha);
}

// S = H(enc(R) || pk || m) * a + r mod L with the context's a and pk   (:404-414)
template <typename Sha = ShaPlain>
C25519_DEV void sign_ctx_s(u32 (&s)[8], const u32 (&encR)[8], const u32* ctx, const uint8_t* msg, size_t len, const u32 (&r)[8],
                           const Sha& sha = Sha())
{
    u32 a[8], pkw[8];
    load32(a, ctx, SCTX_A);
    load32(pkw, ctx, SCTX_PK);
    ed_sign_s(s, encR, pkw, msg, len, a, r, sha);
}

C25519_DEV void sign_ctx_zero_sig(void* sig, size_t e)
{
    const u32 zero[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    store32(sig, 2 * e, zero);
    store32(sig, 2 * e + 1, zero);
}

// ---- one lane per element: k_ed25519_sign_indexed_mult (r, R = r*B), the shared inversion (sig[e][0..31] = enc(R)), then this ----
// r of a bad index is 0 (its walk gives the neutral element, its signature is overwritten with zeros here)
C25519_DEV void sign_ctx_nonce_lane(u32 (&r)[8], const u32* ctx, const Msgs& msgs, size_t i)
{
    if (ctx) {
        sign_ctx_r(r, ctx, msgs.ptr(i), msgs.len(i));
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = 0;
    }
}

// S of element i; the scratch copy of r is zeroed behind the read (the reference clears its r, ed25519_sign.c:417)
C25519_DEV void sign_ctx_finish_lane(void* sig, const u32* ctx, const Msgs& msgs, size_t n, size_t i, u32* r_in)
{
    u32 encR[8], r[8], s[8];
    const u32 zero[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    soa_load8(r, r_in, n, i);
    soa_store8(r_in, n, i, zero);
    if (!ctx) {
        sign_ctx_zero_sig(sig, i);
        return;
    }
    load32(encR, sig, 2 * i);
    sign_ctx_s(s, encR, ctx, msgs.ptr(i), msgs.len(i), r);
    store32(sig, 2 * i + 1, s);
}

namespace quad {

// quad::sign_element with the key from `ctx` (null: 64 zero bytes; the whole quad leaves)
C25519_DEV void sign_ctx_element(void* sig, const u32* ctx, const uint8_t* msg, size_t len, size_t e, const u32* __restrict__ g_wide,
                                 unsigned short* cols, int stride)
{
    const Roles R = roles();
    if (!ctx) {
        if (R.is0) sign_ctx_zero_sig(sig, e);
        return;
    }
    u32 r[8], encR[8], s[8];
    sign_ctx_r(r, ctx, msg, len);
    wb_columns(cols, stride, r);
    fe own;
    base_mult_wide(own, g_wide, cols, stride, R);
    encode_point(encR, own);
    sign_ctx_s(s, encR, ctx, msg, len, r);
    if (R.is0) {
        store32(sig, 2 * e, encR);
        store32(sig, 2 * e + 1, s);
    }
}

}  // namespace quad

namespace coop {

// coop::sign_one with the key from `ctx` (not null: the kernel handles a bad index before the waves split).  Two hashes, so a
// helper wave serves sha512_blocks(4, len) + sha512_blocks(8, len) compressions.
template <bool WIDE, typename Sha = ShaPlain>
C25519_DEV void sign_ctx_one(u32* lds, const Lane& L, void* sig, const u32* ctx, const Msgs& msgs, size_t e, const u32* __restrict__ g_tbl,
                             const DoneWord* done = nullptr, const Sha& sha = Sha())
{
    u32 r[8], xw[8], yw[8], enc[8], s[8];
    sign_ctx_r(r, ctx, msgs.ptr(e), msgs.len(e), sha);
    setup_one(lds, L);
    const u32 v = base_mult_one<WIDE>(lds, L, r, g_tbl, nullptr);
    ge_affine_words(xw, yw, lds, L, v);
    ge_pack(enc, xw, yw);
    sign_ctx_s(s, enc, ctx, msgs.ptr(e), msgs.len(e), r, sha);
    if (threadIdx.x == 0) {
        store32(sig, 2 * e, enc);
        store32(sig, 2 * e + 1, s);
    }
    finish(lds, LDS_WORDS, done);
}

// the compressions of sign_ctx_one's two hashes (the helper wave's count)
C25519_DEV int sign_ctx_sha_blocks(size_t len) { return sha512_blocks(4, len) + sha512_blocks(8, len); }

}  // namespace coop

}  // namespace c25519
