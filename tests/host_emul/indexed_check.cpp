// tests/host_emul/indexed_check.cpp -- TEST INFRASTRUCTURE.  ed25519_Verify_Check against many contexts
// (curve25519_amd/csrc/verify_ctx.cuh: what ed25519_Verify_Check_indexed_* runs on the device) driven on the CPU the way
// engine_verify_ctx.hip drives it: k_ed25519_verify_check_indexed's lane (indexed_ctx, verify_ctx_point over the context's rows in place,
// or over the 128-byte-aligned copy k_ed25519_verify_ctx_repack makes), the projective results in the scratch's SoA layout, then
// k_batch_invert<FinishVerifyIndexed, K>'s lanes (csrc/batch_invert_lane.inc) in workgroups of 64 lock-step lanes.  The contexts are
// copied into a buffer of exactly n_ctx x 2080 bytes first, so that a build with -fsanitize=address sees a read past them.
// Built into its own library by tests/test_host_emul_indexed_check.py through tests/host_emul/build.py's build_lib.
// Not part of the product.
#define EMUL_COOP_WAVE_IMPL 1
#include "coop_wave.h"
#include "lanes.cuh"
#include "batch_invert.cuh"
#include "verify_ctx.cuh"

#include <mutex>
#include <vector>

using namespace c25519;

namespace c25519 { unsigned long long emul_mad_overflows = 0, emul_mad_count = 0; LatCounters emul_lat_counters = { 0, 0, 0 }; }
thread_local EmulWave* emul_wave = nullptr;
thread_local emul_dim3 emul_tid = { 0, 0, 0 };

namespace {

std::mutex g_mu;                        // one emulated workgroup at a time (coop_wave.h)

// the reference's 8-fold base table as k_ed25519_verify_check_indexed stages it in LDS: [30][256] limbs
const u32* ref_table()
{
    static std::vector<u32> t;
    static std::once_flag once;
    std::call_once(once, [] {
        t.assign((size_t)PA_WORDS * 256, 0);
        for (u32 k = 0; k < 256; k++) {
            u32 rows[3][8];
            ge_base_table_row(rows, k, 0);
            for (int f = 0; f < 3; f++) {
                fe c;
                fe_from_words(c, rows[f]);
                for (int l = 0; l < 10; l++) t[(size_t)(10 * f + l) * 256 + k] = c.v[l];
            }
        }
    });
    return t.data();
}

template <typename Fin, int K>
void batch_invert_lane(const u32* Z, u32* pre_lds, size_t n, size_t m, Fin fin, unsigned block)
{
    const emul_dim3 blockIdx = { block, 0, 0 };
#include "batch_invert_lane.inc"
}

template <int K>
void invert_all(const u32* Z, size_t n, const FinishVerifyIndexed& fin)
{
    const size_t m = (n + K - 1) / K;
    std::vector<u32> pre_lds(K > 14 ? (K - 1) * 10 * INV_BLOCK : 1);
    for (unsigned block = 0; (size_t)block * INV_BLOCK < m; block++)
        emul_coop::run_block(INV_BLOCK, [&] { batch_invert_lane<FinishVerifyIndexed, K>(Z, pre_lds.data(), n, m, fin, block); });
}

}  // namespace

extern "C" {

unsigned long long emul_mad_overflow_count(void) { return emul_mad_overflows; }

// verdicts of n pairs against contexts ctx_index[i] of n_ctx; messages ragged (offsets: n + 1 entries) or `len` bytes apart
// (offsets == NULL).  repack: read the rows from an aligned copy.  k: elements per inverting lane.  Returns the group size used.
int emul_indexed_check(int* verdict, const unsigned char* ctxs_in, size_t n_ctx, const unsigned* ctx_index, const unsigned char* sig_in,
                       const unsigned char* msg, size_t len, const unsigned long long* offsets, size_t n, int repack, int k)
{
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<u32> ctxs(n_ctx * VCTX_WORDS), rows(repack ? n_ctx * QTABLE_CANON_WORDS : 0);
    std::vector<u32> sig(16 * n);
    memcpy(ctxs.data(), ctxs_in, n_ctx * VCTX_BYTES);
    memcpy(sig.data(), sig_in, 64 * n);
    for (size_t c = 0; c < rows.size() / QTABLE_CANON_WORDS; c++)                  // k_ed25519_verify_ctx_repack
        memcpy(&rows[c * QTABLE_CANON_WORDS], &ctxs[c * VCTX_WORDS + 8], QTABLE_CANON_WORDS * 4);
    const Msgs msgs{ msg, len, offsets };
    const u32* lds_tbl = ref_table();
    std::vector<u32> X(10 * n), Y(10 * n), Z(10 * n);
    for (size_t i = 0; i < n; i++) {                                                // k_ed25519_verify_check_indexed, lane i
        const u32* ctx = indexed_ctx(ctxs.data(), n_ctx, ctx_index, i);
        const QTableCanon tbl{ repack ? (ctx ? &rows[(size_t)ctx_index[i] * QTABLE_CANON_WORDS] : nullptr) : const_cast<u32*>(ctx) + 8 };
        ge_ext T;
        verify_ctx_point(T, ctx, tbl, sig.data(), msgs, i, lds_tbl);
        soa_store_fe(X.data(), n, i, T.X);
        soa_store_fe(Y.data(), n, i, T.Y);
        soa_store_fe(Z.data(), n, i, T.Z);
    }
    const FinishVerifyIndexed fin{ X.data(), Y.data(), sig.data(), verdict, n, ctx_index, n_ctx };
    const int K = inversion_group(k);
    switch (K) {
    case 16: invert_all<16>(Z.data(), n, fin); break;
    case 14: invert_all<14>(Z.data(), n, fin); break;
    case 12: invert_all<12>(Z.data(), n, fin); break;
    case 8:  invert_all<8>(Z.data(), n, fin); break;
    case 4:  invert_all<4>(Z.data(), n, fin); break;
    case 2:  invert_all<2>(Z.data(), n, fin); break;
    default: invert_all<1>(Z.data(), n, fin); break;
    }
    return K;
}

}  // extern "C"
