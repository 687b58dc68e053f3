// tests/host_emul/taint_sign_ctx.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over sign_ctx.cpp: Ed25519 signing
// against many signer contexts in one call.  Secret: priv[0..31] at Sign_Init; all 128 bytes of every context at
// SignMessage_indexed.  Public: messages, lengths, ctx_index.  The base tables count as secret once built (taint_emul.cpp).
#include "sign_ctx.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    constexpr size_t N_CTX = 3, QUAD_N = quad::ELEMS_PER_WAVE;
    // contexts with a real public half: key pairs from public seeds while the tables are public
    std::vector<unsigned char> seeds = taint::bytes(32 * N_CTX, 91), pub(32 * N_CTX), priv(64 * N_CTX), ctxs(SCTX_BYTES * N_CTX);
    emul_set_base_comb(0);
    emul_ed25519_keypair(pub.data(), priv.data(), nullptr, seeds.data(), N_CTX);
    emul_sign_ctx_init(ctxs.data(), priv.data(), N_CTX);
    taint::secret(ctxs);
    for (size_t n : { (size_t)1, N_CTX }) {
        if (!args.base) break;
        std::vector<unsigned char> p(priv.begin(), priv.begin() + 64 * n), c(SCTX_BYTES * n);
        for (size_t i = 0; i < n; i++) taint::secret(p.data() + 64 * i, 32);
        taint::begin("sign_ctx_init/lane/n%zu", n);
        emul_sign_ctx_init(c.data(), p.data(), n);
    }
    tables();
    wide_tables();
    taint::secret(g_tbl);
    taint::secret(g_wide);
    for (size_t len : args.lens)
        for (int form = 0; form < 3; form++)
            for (int wide = 0; wide < 2; wide++) {
                if (form == 1 && !wide) continue;                                  // the quads always walk the wide comb
                for (size_t n : { (size_t)1, (size_t)5, QUAD_N }) {
                    if (form == 0 ? n == QUAD_N : form == 1 ? n != QUAD_N : n != 1) continue;
                    std::vector<unsigned> index(n);
                    for (size_t i = 0; i < n; i++) index[i] = (unsigned)((i + len) % N_CTX);
                    std::vector<unsigned char> msg = taint::bytes(len * n + 1, 92), sig(64 * n);
                    taint::begin("sign_indexed/%s/%s/n%zu/len%zu", form == 0 ? "lane" : form == 1 ? "quad" : "wave", wide ? "wide" : "comb", n, len);
                    emul_sign_indexed(sig.data(), ctxs.data(), N_CTX, index.data(), msg.data(), len, nullptr, n, form, wide);
                }
            }
}
