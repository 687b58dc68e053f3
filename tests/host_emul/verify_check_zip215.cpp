// tests/host_emul/verify_check_zip215.cpp -- TEST INFRASTRUCTURE.  The coset comparison of ed25519_Verify_Check_zip215_*
// (curve25519_amd/csrc/verify_ctx_zip215.cuh) driven on the CPU the way engine_verify_ctx.hip drives it behind the walk: the coset prep's
// lane (coset_prep_element) over projective points in the scratch's SoA layout, then k_batch_invert<FinishVerifyZip215, K>'s lanes
// (csrc/batch_invert_lane.inc) over the products it left, in workgroups of 64 lock-step lanes; and the per-context rule 2
// (zip215_ctx_key_ok).  The points come from the caller (tests/check_zip215_model.py computes T = [S]B - [k]A in big integers and
// scales it by a Z of its choice), so the walk itself -- tests/host_emul/indexed_check.cpp's subject -- is not run again here.
// Built into its own library by tests/test_host_emul_verify_check_zip215.py through tests/host_emul/build.py's build_lib.
// Not part of the product.
#define EMUL_COOP_WAVE_IMPL 1
#include "coop_wave.h"
#include "lanes.cuh"
#include "batch_invert.cuh"
#include "verify_ctx_zip215.cuh"

#include <mutex>
#include <vector>

using namespace c25519;

namespace c25519 { unsigned long long emul_mad_overflows = 0, emul_mad_count = 0; LatCounters emul_lat_counters = { 0, 0, 0 }; }
thread_local EmulWave* emul_wave = nullptr;
thread_local emul_dim3 emul_tid = { 0, 0, 0 };

namespace {

std::mutex g_mu;                        // one emulated workgroup at a time (coop_wave.h)

template <typename Fin, int K>
void batch_invert_lane(const u32* Z, u32* pre_lds, size_t n, size_t m, Fin fin, unsigned block)
{
    const emul_dim3 blockIdx = { block, 0, 0 };
#include "batch_invert_lane.inc"
}

template <int K>
void invert_all(const u32* W, size_t n, const FinishVerifyZip215& fin)
{
    const size_t m = (n + K - 1) / K;
    std::vector<u32> pre_lds(K > 14 ? (K - 1) * 10 * INV_BLOCK : 1);
    for (unsigned block = 0; (size_t)block * INV_BLOCK < m; block++)
        emul_coop::run_block(INV_BLOCK, [&] { batch_invert_lane<FinishVerifyZip215, K>(W, pre_lds.data(), n, m, fin, block); });
}

}  // namespace

extern "C" {

unsigned long long emul_mad_overflow_count(void) { return emul_mad_overflows; }

// rule 2 from a 2080-byte context
unsigned emul_zip215_ctx_key_ok(const unsigned char* ctx_in)
{
    std::vector<u32> ctx(VCTX_WORDS);
    memcpy(ctx.data(), ctx_in, VCTX_BYTES);
    return zip215_ctx_key_ok(ctx.data());
}

// verdicts of n elements whose walk left (X : Y : Z) = xyz[i] (3 x 32 bytes each, any value below 2^255): coset prep, shared
// inversion with k elements per lane, finish.  ctx_index may be null (one context).  Returns the group size used.
int emul_check_zip215_finish(int* verdict, const unsigned char* xyz, const unsigned* ctx_index, size_t n_ctx, const unsigned* key_ok,
                             const unsigned char* sig_in, size_t n, int k)
{
    std::lock_guard<std::mutex> lk(g_mu);
    std::vector<u32> sig(16 * n), X(10 * n), Y(10 * n), Z(10 * n), W(10 * n);
    memcpy(sig.data(), sig_in, 64 * n);
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        fe f;
        u32* const dst[3] = { X.data(), Y.data(), Z.data() };
        for (int c = 0; c < 3; c++) {
            memcpy(w, xyz + 96 * i + 32 * c, 32);
            fe_from_words(f, w);
            soa_store_fe(dst[c], n, i, f);
        }
    }
    for (size_t i = 0; i < n; i++) coset_prep_element(W.data(), X.data(), Y.data(), Z.data(), n, i);      // the coset prep kernel, lane i
    const FinishVerifyZip215 fin{ X.data(), Y.data(), Z.data(), sig.data(), verdict, n, ctx_index, n_ctx, key_ok };
    const int K = inversion_group(k < 12 ? k : 12);         // (launch_coset_finish: this finish goes up to 12)
    switch (K) {
    case 12: invert_all<12>(W.data(), n, fin); break;
    case 8:  invert_all<8>(W.data(), n, fin); break;
    case 4:  invert_all<4>(W.data(), n, fin); break;
    case 2:  invert_all<2>(W.data(), n, fin); break;
    default: invert_all<1>(W.data(), n, fin); break;
    }
    return K;
}

}  // extern "C"
