// tests/host_emul/peer_ctx.cpp -- TEST INFRASTRUCTURE.  X25519 against many peer contexts (curve25519_amd/csrc/x25519_peer_ctx.cuh:
// what curve25519_dh_Peer_Init_* and curve25519_dh_CreateSharedKey_indexed_* run on the device) driven on the CPU the way
// engine_x25519.hip drives it: k_x25519_peer_init's peer_ctx_build per key, then k_x25519_peer_indexed_walk's lane (peer_ctx_of, the
// ladder list for an ineligible context, peer_ctx_columns + peer_ctx_walk over the context's rows in place), k_x25519_peer_indexed_ladder
// for the listed elements, and the shared inversion as a plain fe_invert (0 for 0, as k_batch_invert gives).  The contexts are copied
// into a buffer of exactly n_ctx x 1600 bytes first, so that a build with -fsanitize=address sees a read past them.
// Built into its own library by tests/test_host_emul_peer_ctx.py through tests/host_emul/build.py's build_lib.  Not part of the product.
#define EMUL_COOP_WAVE_IMPL 1
#include "coop_wave.h"
#include "lanes.cuh"
#include "x25519_peer_ctx.cuh"

#include <thread>
#include <vector>

using namespace c25519;

namespace c25519 { unsigned long long emul_mad_overflows = 0, emul_mad_count = 0; LatCounters emul_lat_counters = { 0, 0, 0 }; }
thread_local EmulWave* emul_wave = nullptr;
thread_local emul_dim3 emul_tid = { 0, 0, 0 };

namespace {

void rd32(u32 (&w)[8], const unsigned char* p, size_t i) { memcpy(w, p + 32 * i, 32); }
void wr32(unsigned char* p, size_t i, const u32 (&w)[8]) { memcpy(p + 32 * i, w, 32); }

template <typename F>
void parallel_for(size_t n, F f)
{
    const size_t T = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (size_t t = 0; t < T; t++)
        pool.emplace_back([&, t] { for (size_t i = t; i < n; i += T) f(i); });
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" {

unsigned long long emul_mad_overflow_count(void) { return emul_mad_overflows; }

// curve25519_dh_Peer_Init for n keys: n x 1600 bytes to ctx_out
void emul_peer_init(unsigned char* ctx_out, const unsigned char* pk, size_t n)
{
    std::vector<u32> ctxs(n * PEER_CTX_WORDS);
    parallel_for(n, [&](size_t i) {
        u32 u[8];
        rd32(u, pk, i);
        std::vector<u32> tbl(QTABLE_LIMB_WORDS);
        peer_ctx_build(&ctxs[i * PEER_CTX_WORDS], u, tbl.data());
    });
    memcpy(ctx_out, ctxs.data(), n * PEER_CTX_BYTES);
}

// curve25519_dh_CreateSharedKey_indexed_dev for n secrets against contexts ctx_index[i] of n_ctx, sk clamped in place.  Returns the
// number of elements that ran the ladder (k_x25519_peer_indexed_ladder's report).
long emul_peer_indexed(unsigned char* out, const unsigned char* ctxs_in, size_t n_ctx, const unsigned* ctx_index, unsigned char* sk,
                       size_t n)
{
    std::vector<u32> ctxs(n_ctx * PEER_CTX_WORDS);
    memcpy(ctxs.data(), ctxs_in, n_ctx * PEER_CTX_BYTES);
    std::vector<u32> num(10 * n), den(10 * n), list(n);
    u32 count = 0;
    for (size_t i = 0; i < n; i++) {                                   // the walk kernel's lane prologue: clamp, the ladder list
        u32 k[8];
        rd32(k, sk, i);
        clamp_words(k);
        wr32(sk, i, k);
        const u32* ctx = peer_ctx_of(ctxs.data(), n_ctx, ctx_index, i);
        if (ctx && ctx[PEER_CTX_ELIGIBLE] != 1u) list[atomicAdd(&count, 1u)] = (u32)i;
    }
    parallel_for(n, [&](size_t i) {                                    // ... and its walk
        const u32* ctx = peer_ctx_of(ctxs.data(), n_ctx, ctx_index, i);
        if (ctx && ctx[PEER_CTX_ELIGIBLE] != 1u) return;
        u32 k[8], cols[8];
        rd32(k, sk, i);
        fe N, D;
        if (ctx) {
            peer_ctx_columns(cols, 1, k);
            peer_ctx_walk(N, D, cols, 1, ctx + PEER_CTX_ROWS);
        } else {
            fe_set_u32(N, 0);
            fe_set_u32(D, 0);
        }
        soa_store_fe(num.data(), n, i, N);
        soa_store_fe(den.data(), n, i, D);
    });
    parallel_for(count, [&](size_t j) {                                // k_x25519_peer_indexed_ladder
        const size_t i = list[j];
        u32 u[8], k[8];
        peer_ctx_key(u, ctxs.data() + (size_t)ctx_index[i] * PEER_CTX_WORDS);
        rd32(k, sk, i);
        fe PX, PZ;
        x25519_ladder_xz<false>(PX, PZ, u, k);
        soa_store_fe(num.data(), n, i, PX);
        soa_store_fe(den.data(), n, i, PZ);
    });
    parallel_for(n, [&](size_t i) {                                    // FinishX25519 behind the shared inversion
        fe N, D, zi;
        u32 w[8];
        soa_load_fe(N, num.data(), n, i);
        soa_load_fe(D, den.data(), n, i);
        fe_invert(zi, D);
        fe_mul(N, N, zi);
        fe_to_words(w, N);
        wr32(out, i, w);
    });
    return (long)count;
}

// k_x25519_peer_gather: the key of each element's context, 32 zero bytes for an index >= n_ctx
void emul_peer_gather(unsigned char* keys, const unsigned char* ctxs_in, size_t n_ctx, const unsigned* ctx_index, size_t n)
{
    std::vector<u32> ctxs(n_ctx * PEER_CTX_WORDS);
    memcpy(ctxs.data(), ctxs_in, n_ctx * PEER_CTX_BYTES);
    for (size_t i = 0; i < n; i++) {
        u32 u[8];
        peer_ctx_key(u, peer_ctx_of(ctxs.data(), n_ctx, ctx_index, i));
        wr32(keys, i, u);
    }
}

}  // extern "C"
