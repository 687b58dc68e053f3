// tests/host_emul/one_peer.cpp -- TEST INFRASTRUCTURE.  X25519 against ONE peer key (curve25519_amd/csrc/x25519_peer.cuh)
// driven on the CPU the way engine_x25519.hip drives it per lane: k_x25519_peer_check's x25519_peer_point, the rows of the peer's
// comb from k_x25519_peer_prepare's ge_signed_comb_row_of at the offsets that kernel writes them to, and k_x25519_one_peer_mult's
// x25519_one_peer_lane over them; the shared inversion is a plain fe_invert.  A comb row costs ~2400 field operations in the
// C model, so only the rows the secrets of a call select are generated (all of them would be 16384 per peer); the walk reads
// them from a full-size table in the device layout.  Built into its own library by tests/test_host_emul_one_peer.py through
// tests/host_emul/build.py's build_lib.  Not part of the product.
#define EMUL_COOP_WAVE_IMPL 1
#include "coop_wave.h"
#include "lanes.cuh"
#include "x25519_peer.cuh"

#include <thread>
#include <vector>

using namespace c25519;

namespace c25519 { unsigned long long emul_mad_overflows = 0, emul_mad_count = 0; LatCounters emul_lat_counters = { 0, 0, 0 }; }
thread_local EmulWave* emul_wave = nullptr;
thread_local emul_dim3 emul_tid = { 0, 0, 0 };

namespace {

void rd32(u32 (&w)[8], const unsigned char* p, size_t i) { memcpy(w, p + 32 * i, 32); }
void wr32(unsigned char* p, size_t i, const u32 (&w)[8]) { memcpy(p + 32 * i, w, 32); }

// f(i) for i in [0, n) on a few host threads
template <typename F>
void parallel_for(size_t n, F f)
{
    const size_t T = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (size_t t = 0; t < T; t++)
        pool.emplace_back([&, t] { for (size_t i = t; i < n; i += T) f(i); });
    for (auto& th : pool) th.join();
}

// the table row (table * WB_ROWS + row) a column selects in table t: wb_load_pa_signed's index
size_t row_of(int t, u32 c)
{
    const u32 neg = ((c >> (WB_TEETH - 1)) & 1u) - 1u;
    return (size_t)t * WB_ROWS + ((c ^ neg) & (u32)(WB_ROWS - 1));
}

}  // namespace

extern "C" {

unsigned long long emul_mad_overflow_count(void) { return emul_mad_overflows; }

// k_x25519_peer_check for a new peer: Q = 8P as 96 canonical bytes (Y+X | Y-X | 2dT), returns the eligibility word (1 / 0)
int emul_one_peer_point(unsigned char* q_out, const unsigned char* pk)
{
    u32 u[8], q[3][8];
    rd32(u, pk, 0);
    const u32 ok = x25519_peer_point(q, u);
    memcpy(q_out, q, 96);
    return ok ? 1 : 0;
}

// rows idx[i] (table * WB_ROWS + row) of the comb of the point whose 96 bytes q_in holds, as k_x25519_peer_prepare writes them
// (32 words each: three canonical fields, then 2, 0, ...)
void emul_one_peer_rows(unsigned* out, const unsigned char* q_in, const unsigned* idx, size_t n)
{
    u32 qw[PEER_Q_WORDS];
    memcpy(qw, q_in, sizeof qw);
    ge_pa Q;
    x25519_peer_pa(Q, qw);
    parallel_for(n, [&](size_t i) {
        const u32 g = idx[i];
        const int table = (int)(g / WB_ROWS);
        u32 rows[3][8];
        ge_signed_comb_row_of(rows, Q, g % WB_ROWS, (WB_NT - 1 - table) * WB_STEP, WB_TEETH, WB_COLS);
        u32* o = out + i * WB_ROW_WORDS;
        memset(o, 0, WB_ROW_WORDS * 4);
        memcpy(o, rows, 96);
        o[24] = 2;
    });
}

// the peer's comb in the device layout with only the rows that the n clamped secrets k (8 words each) select: the columns of every
// secret (k >> 3, as x25519_one_peer_lane recodes it), then the rows of those columns by emul_one_peer_rows
static void one_peer_needed_rows(std::vector<u32>& wide_peer, const u32 (&q)[3][8], const std::vector<u32>& k, size_t n)
{
    std::vector<unsigned short> cols(WB_COLS * n);
    for (size_t i = 0; i < n; i++) {
        u32 kw[8], k3[8];
        memcpy(kw, &k[8 * i], 32);
        for (int j = 0; j < 7; j++) k3[j] = (kw[j] >> 3) | (kw[j + 1] << 29);
        k3[7] = kw[7] >> 3;
        wb_columns(&cols[WB_COLS * i], 1, k3);
    }
    std::vector<char> need((size_t)WB_NT * WB_ROWS, 0);
    for (size_t i = 0; i < n; i++)
        for (int m = 0; m < WB_STEP; m++)
            for (int t = 0; t < WB_NT; t++) need[row_of(t, cols[WB_COLS * i + m * WB_NT + t])] = 1;
    std::vector<unsigned> idx;
    for (size_t g = 0; g < need.size(); g++)
        if (need[g]) idx.push_back((unsigned)g);
    std::vector<u32> rows(idx.size() * WB_ROW_WORDS);
    wide_peer.assign(WB_TBL_WORDS, 0);
    emul_one_peer_rows(rows.data(), reinterpret_cast<const unsigned char*>(q), idx.data(), idx.size());
    for (size_t r = 0; r < idx.size(); r++) memcpy(&wide_peer[(size_t)idx[r] * WB_ROW_WORDS], &rows[r * WB_ROW_WORDS], WB_ROW_WORDS * 4);
}

// curve25519_dh_CreateSharedKey_one_peer for n secrets against the one key pk, sk clamped in place.  Returns 1 if the comb decided
// (the peer is eligible), 0 if the ladder did (x25519_ladder_xz per secret, as k_x25519_ladder_one_peer).
int emul_one_peer(unsigned char* out, const unsigned char* pk, unsigned char* sk, size_t n)
{
    u32 u[8], q[3][8];
    rd32(u, pk, 0);
    const bool wide = x25519_peer_point(q, u) != 0;
    std::vector<u32> k(8 * n);
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        rd32(w, sk, i);
        clamp_words(w);
        wr32(sk, i, w);
        memcpy(&k[8 * i], w, 32);
    }
    if (!wide) {
        parallel_for(n, [&](size_t i) {
            u32 kw[8], w[8];
            memcpy(kw, &k[8 * i], 32);
            fe PX, PZ, zi;
            x25519_ladder_xz<false>(PX, PZ, u, kw);
            fe_invert(zi, PZ);
            fe_mul(PX, PX, zi);
            fe_to_words(w, PX);
            wr32(out, i, w);
        });
        return 0;
    }
    std::vector<u32> wide_peer;
    one_peer_needed_rows(wide_peer, q, k, n);
    std::vector<unsigned short> cols(WB_COLS * n);
    parallel_for(n, [&](size_t i) {
        u32 kw[8], w[8];
        memcpy(kw, &k[8 * i], 32);
        fe num, den, zi;
        x25519_one_peer_lane(num, den, kw, wide_peer.data(), &cols[WB_COLS * i], 1);
        fe_invert(zi, den);                                  // fe_invert(0) = 0: the shared inversion's answer for a zero denominator
        fe_mul(num, num, zi);
        fe_to_words(w, num);
        wr32(out, i, w);
    });
    return 1;
}

}  // extern "C"
