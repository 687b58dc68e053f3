// tests/host_emul/sign_ctx.cpp -- TEST INFRASTRUCTURE.  Ed25519 signing against many signer contexts (curve25519_amd/csrc/sign_ctx.cuh:
// what ed25519_Sign_Init_* and ed25519_SignMessage_indexed_* run on the device) driven on the CPU the way engine_fixed_base.hip
// drives it: k_ed25519_sign_ctx_init's lane per key; then one of the three signing forms --
//   form 0  one lane per element: k_ed25519_sign_indexed_mult's lane (sign_ctx_of, sign_ctx_nonce_lane, r to the scratch's SoA
//           layout, r*B over the LDS comb's tables or the wide comb), the shared inversion as a plain affine encoding (FinishPack's
//           sig[e][0..31] = enc(R)), k_ed25519_sign_indexed_finish's lane (sign_ctx_finish_lane);
//   form 1  four lanes per element: k_ed25519_sign_indexed_quad's quads of one 64-lane wave (quad::sign_ctx_element);
//   form 2  one element per two-wave workgroup: k_ed25519_sign_indexed_coop (the helper wave serving the SHA-512 schedules).
// The contexts are copied into a buffer of exactly n_ctx x 128 bytes first, so that a build with -fsanitize=address sees a read past
// them.  The base tables, the wide comb and the lock-step lane scheduler come from emul.cpp, included whole: this file is its own
// library (tests/test_host_emul_sign_indexed.py, through tests/host_emul/build.py's build_lib).  Not part of the product.
#include "emul.cpp"
#include "sign_ctx.cuh"

namespace {

std::vector<u32> copy_ctxs(const unsigned char* ctxs_in, size_t n_ctx)
{
    std::vector<u32> ctxs(n_ctx * SCTX_WORDS);
    memcpy(ctxs.data(), ctxs_in, n_ctx * SCTX_BYTES);
    return ctxs;
}

}  // namespace

extern "C" {

// ed25519_Sign_Init for n keys: n x 128 bytes to ctx_out
void emul_sign_ctx_init(unsigned char* ctx_out, const unsigned char* priv_in, size_t n)
{
    std::vector<u32> priv(16 * n), ctxs(n * SCTX_WORDS);
    memcpy(priv.data(), priv_in, 64 * n);
    for (size_t i = 0; i < n; i++) sign_ctx_init_lane(ctxs.data(), priv.data(), i);
    memcpy(ctx_out, ctxs.data(), n * SCTX_BYTES);
}

// n signatures under contexts ctx_index[i] of n_ctx; messages ragged (offsets: n + 1 entries) or `len` bytes apart (offsets ==
// NULL).  form: 0 one lane, 1 quad, 2 per wave.  wide: the wide comb (forms 0 and 2; the quad form always walks it).
void emul_sign_indexed(unsigned char* sig_out, const unsigned char* ctxs_in, size_t n_ctx, const unsigned* ctx_index,
                       const unsigned char* msg, size_t len, const unsigned long long* offsets, size_t n, int form, int wide)
{
    std::lock_guard<std::mutex> lk(g_coop_mu);
    const std::vector<u32> ctxs = copy_ctxs(ctxs_in, n_ctx);
    std::vector<u32> sig(16 * n, 0xa5a5a5a5u);
    const Msgs msgs{ msg, len, offsets };
    if (form == 0) {
        std::vector<u32> r_buf(8 * n);
        for (size_t i = 0; i < n; i++) {                                            // k_ed25519_sign_indexed_mult, lane i
            u32 r[8], enc[8];
            sign_ctx_nonce_lane(r, sign_ctx_of(ctxs.data(), n_ctx, ctx_index, i), msgs, i);
            soa_store8(r_buf.data(), n, i, r);
            ge_ext S;
            if (wide) base_mult_wide(S, r, nullptr, false);
            else ge_base_mult(S, r, tables());
            affine_pack_host(enc, S);                                               // the shared inversion's FinishPack
            store32(sig.data(), 2 * i, enc);
        }
        for (size_t i = 0; i < n; i++)                                              // k_ed25519_sign_indexed_finish, lane i
            sign_ctx_finish_lane(sig.data(), sign_ctx_of(ctxs.data(), n_ctx, ctx_index, i), msgs, n, i, r_buf.data());
        for (u32 w : r_buf)
            if (w) abort();                                                          // r is wiped behind its read
    } else if (form == 1) {
        const u32* g_wide = wide_tables();
        std::vector<unsigned short> cols(WB_COLS * 64);
        for (size_t base = 0; base < n; base += quad::ELEMS_PER_WAVE)
            emul_coop::run_block(64, [&] {
                const size_t e = base + (threadIdx.x >> 2);
                if (e >= n) return;
                quad::sign_ctx_element(sig.data(), sign_ctx_of(ctxs.data(), n_ctx, ctx_index, e), msgs.ptr(e), msgs.len(e), e, g_wide,
                                       cols.data() + threadIdx.x, 64);
            });
    } else {
        std::vector<u32> lds(coop::LDS_WORDS);
        std::vector<u64> sha_wk(80);
        const u32* tbl = wide ? wide_tables() : tables();
        for (size_t e = 0; e < n; e++)
            emul_coop::run_block(128, [&] {
                const u32* ctx = sign_ctx_of(ctxs.data(), n_ctx, ctx_index, e);
                if (!ctx) {
                    if (threadIdx.x == 0) sign_ctx_zero_sig(sig.data(), e);
                    return;
                }
                if (threadIdx.x >= 64) { coop::sha_schedule_server(sha_wk.data(), coop::sign_ctx_sha_blocks(msgs.len(e))); return; }
                const coop::Lane L = coop::make_lane(threadIdx.x);
                const coop::ShaTwoWaves sha{ sha_wk.data() };
                if (wide) coop::sign_ctx_one<true>(lds.data(), L, sig.data(), ctx, msgs, e, tbl, nullptr, sha);
                else coop::sign_ctx_one<false>(lds.data(), L, sig.data(), ctx, msgs, e, tbl, nullptr, sha);
            });
    }
    memcpy(sig_out, sig.data(), 64 * n);
}

}  // extern "C"
