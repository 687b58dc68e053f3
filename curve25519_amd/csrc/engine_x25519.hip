// curve25519_amd/csrc/engine_x25519.hip -- the X25519 kernels (the Montgomery ladder per lane, fused with the shared inversion, per wave, on two
// waves, on quads; many secrets against one peer key over that key's wide comb) and curve25519_dh_CreateSharedKey_dev /
// curve25519_dh_CalculatePublicKey_dev / curve25519_dh_CreateSharedKey_one_peer_dev
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "x25519_peer.cuh"
#include "x25519_peer_ctx.cuh"

// ------------------------------------------------------------------------------------------------
// X25519   (curve25519_dh_CreateSharedKey / curve25519_dh_CalculatePublicKey)
// ------------------------------------------------------------------------------------------------
// Single launch: the eight waves of a workgroup finish their ladders, park (PX, PZ) in LDS, and wave 0 inverts all
// the workgroup's Z's with ONE exponentiation (eight elements per lane, Montgomery's trick, prefix products in LDS);
// then every lane finishes its own element.  The projective intermediates never leave the CU: HBM traffic is the
// API's 96 B/op plus the clamped-key write-back.   BASE9 (pk == nullptr): ladder on the base point u = 9.
#ifndef C25519_XF_BLOCK
#define C25519_XF_BLOCK 512
#endif
#ifndef C25519_XF_WAVES
#define C25519_XF_WAVES 4             // waves per SIMD the register allocator aims at (A/B: profiles/r02_ab_occupancy.txt)
#endif
constexpr int XF_BLOCK = C25519_XF_BLOCK;     // waves per workgroup = elements per inverting lane

// Opt-in measurement build (tools/cycle_probe.py; never the product): -DC25519_CYCLE_PROBE=1 makes every wave of
// k_x25519_fused stamp s_memtime (one tick = one shader cycle) at its phase boundaries -- entry, end of the ladder, behind
// the first barrier, behind the shared inversion, behind the second barrier, exit -- with the hardware slot it ran on,
// so that cycles per ladder step, the idle time of a workgroup's waves during the inversion and the clock of an
// UN-PROFILED run (kernel wall time / cycles) can be read; =2 additionally accumulates the ten sections of a ladder step.
#ifdef C25519_CYCLE_PROBE
constexpr int PROBE_WORDS = 20;
__device__ unsigned long long* g_cycle_probe = nullptr;
C25519_DEV unsigned long long probe_now()
{
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    return t;
}
// the constant 100 MHz counter: (shader cycles) / (these ticks) * 100 MHz is the shader clock the wave ran at, with no
// host-side timing involved
C25519_DEV unsigned long long probe_realtime()
{
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    return t;
}
struct SectionTimer {
    unsigned long long *last, *acc;
    C25519_DEV void operator()(int id) const
    {
#if C25519_CYCLE_PROBE >= 2
        C25519_SCHED_FENCE();
        const unsigned long long t = probe_now();
        if (id >= 0) acc[id] += t - *last;
        *last = t;
        C25519_SCHED_FENCE();
#endif
    }
};
#define C25519_PROBE_STAMP(i) do { C25519_SCHED_FENCE(); probe_t[i] = probe_now(); C25519_SCHED_FENCE(); } while (0)
#else
#define C25519_PROBE_STAMP(i) do { } while (0)
#endif

// BLOCK lanes per workgroup = 64 x the elements per inverting lane.  XF_BLOCK (512) is the throughput shape; a batch that
// does not fill the chip with it runs narrower workgroups (x25519_block_for): 2^14 elements are 32 workgroups of 512 -- 32
// of 256 CUs, two waves per SIMD -- but 256 of 64, one wave on a SIMD of its own, which finishes in little more than half
// the time; the price, an inversion per 1 / 2 / 4 elements instead of 8, is 2-8 % more instructions.
template <bool BASE9, int BLOCK>
__global__ void __launch_bounds__(BLOCK, C25519_XF_WAVES) k_x25519_fused(void* out, const void* pk, void* sk, size_t n)
{
    constexpr int K = BLOCK / 64;            // elements per lane of the inverting wave
    __shared__ u32 zbuf[10 * BLOCK];      // PZ, later 1/PZ
    __shared__ u32 xbuf[10 * BLOCK];      // PX
    __shared__ u32 pbuf[(K > 1 ? K - 1 : 1) * 10 * 64];   // prefix products of the inverting wave
    const int tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * BLOCK + tid;
    const bool active = i < n;
#ifdef C25519_CYCLE_PROBE
    unsigned long long probe_t[6] = {}, probe_sec[10] = {}, probe_last = 0;
    const unsigned long long probe_rt0 = probe_realtime();
#endif
    C25519_PROBE_STAMP(0);
    {
        fe PX, PZ;
        if (active) {
            u32 u[8] = { 9, 0, 0, 0, 0, 0, 0, 0 }, k[8];
            if (!BASE9) load32(u, pk, i);
            load32(k, sk, i);
            clamp_words(k);
            store32(sk, i, k);                   // the reference clamps in the caller's buffer
#ifdef C25519_CYCLE_PROBE
            x25519_ladder_xz<BASE9>(PX, PZ, u, k, SectionTimer{ &probe_last, probe_sec });
#else
            x25519_ladder_xz<BASE9>(PX, PZ, u, k);
#endif
        } else {
            fe_set_u32(PX, 0);
            fe_set_u32(PZ, 1);
        }
        C25519_PROBE_STAMP(1);
        lds_put_fe(zbuf, BLOCK, tid, PZ);
        lds_put_fe(xbuf, BLOCK, tid, PX);
    }
    __syncthreads();
    C25519_PROBE_STAMP(2);
    if (tid < 64) {
        fe acc, z, zero;
        fe_set_u32(zero, 0);
        u32 zero_mask = 0;
#pragma unroll 1
        for (int t = 0; t < K; t++) {
            lds_get_fe(z, zbuf, BLOCK, tid + 64 * t);
            zero_mask |= (fe_zero_to_one(z) & 1u) << t;
            if (t == 0) acc = z; else fe_mul(acc, acc, z);
            if (t < K - 1) lds_put_fe(pbuf + t * 640, 64, tid, acc);
        }
        fe inv;
        {   // one inversion per quad of the wave's lanes (k_batch_invert's exchange, engine_common.cuh)
            fe partner, pair, other_pair, total;
            quad::fe_qperm<1, 0, 3, 2>(partner, acc);
            fe_mul(pair, acc, partner);
            quad::fe_qperm<2, 3, 0, 1>(other_pair, pair);
            fe_mul(total, pair, other_pair);
            fe_invert_quad(inv, total);
            fe_mul(inv, inv, other_pair);
            fe_mul(inv, inv, partner);
        }
#pragma unroll 1
        for (int t = K - 1; t >= 0; t--) {
            fe zi;
            const u32 was_zero = ((zero_mask >> t) & 1u) ? 0xffffffffu : 0u;
            if (t > 0) {
                fe p;
                lds_get_fe(p, pbuf + (t - 1) * 640, 64, tid);
                fe_mul(zi, inv, p);
                lds_get_fe(z, zbuf, BLOCK, tid + 64 * t);
                fe one;
                fe_set_u32(one, 1);
                fe_select(z, was_zero, one, z);
                fe_mul(inv, inv, z);
                fe_select(zi, was_zero, zero, zi);
            } else {
                fe_select(zi, was_zero, zero, inv);
            }
            lds_put_fe(zbuf, BLOCK, tid + 64 * t, zi);
        }
    }
    C25519_PROBE_STAMP(3);
    __syncthreads();
    C25519_PROBE_STAMP(4);
    if (active) {
        fe x, zi;
        u32 w[8];
        lds_get_fe(x, xbuf, BLOCK, tid);
        lds_get_fe(zi, zbuf, BLOCK, tid);
        fe_mul(x, x, zi);
        fe_to_words(w, x);
        store32(out, i, w);                      // written last: `out` may alias `pk`
    }
#ifdef C25519_CYCLE_PROBE
    C25519_PROBE_STAMP(5);
    if ((tid & 63) == 0 && g_cycle_probe) {
        unsigned long long* rec = g_cycle_probe + ((size_t)blockIdx.x * (BLOCK / 64) + tid / 64) * PROBE_WORDS;
        for (int q = 0; q < 6; q++) rec[q] = probe_t[q];
        // HW_ID (wave / SIMD / CU / SH / SE slot) and XCC_ID of the wave
        rec[6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
        for (int q = 0; q < 10; q++) rec[7 + q] = probe_sec[q];
        rec[17] = probe_rt0;
        rec[18] = probe_realtime();
    }
#endif
}

// The ladder alone: (PX : PZ) to the struct-of-arrays scratch, for k_batch_invert<FinishX25519> behind it.  No LDS, no
// barrier: every wave is on its own, a finished wave's slot goes to the next workgroup at once.  (k_x25519_fused parks
// seven of a workgroup's eight waves at a barrier while wave 0 inverts -- and as every workgroup of a full launch takes
// the same time, both workgroups of a CU get there together: tools/cycle_probe.py, profiles/r04_cycle_probe.txt.)
constexpr int XL_BLOCK = 256;
template <bool BASE9>
__global__ void __launch_bounds__(XL_BLOCK, C25519_XF_WAVES) k_x25519_ladder(u32* X, u32* Z, const void* pk, void* sk, size_t n)
{
    const size_t i = (size_t)blockIdx.x * XL_BLOCK + threadIdx.x;
    if (i >= n) return;
#ifdef C25519_CYCLE_PROBE
    unsigned long long probe_t[6] = {};
    const unsigned long long probe_rt0 = probe_realtime();
#endif
    C25519_PROBE_STAMP(0);
    u32 u[8] = { 9, 0, 0, 0, 0, 0, 0, 0 }, k[8];
    if (!BASE9) load32(u, pk, i);
    load32(k, sk, i);
    clamp_words(k);
    store32(sk, i, k);                           // the reference clamps in the caller's buffer
    fe PX, PZ;
    x25519_ladder_xz<BASE9>(PX, PZ, u, k);
    C25519_PROBE_STAMP(1);
    soa_store_fe(X, n, i, PX);
    soa_store_fe(Z, n, i, PZ);
#ifdef C25519_CYCLE_PROBE
    C25519_PROBE_STAMP(5);
    if ((threadIdx.x & 63) == 0 && g_cycle_probe) {
        unsigned long long* rec = g_cycle_probe + (i / 64) * PROBE_WORDS;
        probe_t[2] = probe_t[3] = probe_t[4] = probe_t[1];
        for (int q = 0; q < 6; q++) rec[q] = probe_t[q];
        rec[6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
        rec[17] = probe_rt0;
        rec[18] = probe_realtime();
    }
#endif
}

// One operation per WAVE (coop25519.cuh): what a call of a few elements runs -- the reference's own single-call
// prototypes above all.  Ladder, doublings, inversion and the last multiplication are cooperative (a field element
// limb-per-lane, up to four products at a time); only the decoding of the inputs and the canonical encoding of the result
// are the batch kernels' per-lane code, run by every lane on the same values.
template <bool BASE9>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4))) k_x25519_coop(void* out, const void* pk, void* sk, size_t n, DoneWord done, CallWords cw)
{
    __shared__ __attribute__((aligned(16))) u32 lds[coop::ROWQ_OFF];
    if (blockIdx.x >= n) return;
    coop::x25519_one<BASE9>(lds, coop::make_lane(threadIdx.x), out, pk, sk, blockIdx.x, &cw, &done);    // (signals behind the result, before its LDS wipe)
}

// ... and on TWO waves per element (coop::x25519_two_waves: a ladder step in two product levels -- the differential addition with
// x1 times the sum carried along on one wave, the doubling on the other, one workgroup barrier per step): what ONE
// curve25519_dh_CreateSharedKey call and calls of up to 512 run -- 183 -> 168 us per call
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(1, 4))) k_x25519_coop2(void* out, const void* pk, void* sk, size_t n, DoneWord done, CallWords cw)
{
    __shared__ __attribute__((aligned(16))) u32 lds[coop::X2_LDS_WORDS];
    if (blockIdx.x >= n) return;
    coop::x25519_two_waves(lds, out, pk, sk, blockIdx.x, &cw, &done);    // (wave 0 stores, signals, wipes; wave 1 has left inside)
}

// FOUR LANES per element (quad25519.cuh): what a call of 2^12 .. 2^14 elements runs -- too many for a wave each, too few to
// give every SIMD a wave of one-lane elements (2^14 elements are 256 such waves on 1024 SIMDs).  A quad runs one product of a
// ladder step per lane and level, operands exchanged with v_mov_b32_dpp quad_perm; 16 elements per wave, one wave per
// workgroup, inversion and encoding in the same launch: no LDS, no scratch, no barrier.
template <bool BASE9>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) k_x25519_quad(void* out, const void* pk, void* sk, size_t n)
{
    const size_t e = (size_t)blockIdx.x * quad::ELEMS_PER_WAVE + (threadIdx.x >> 2);
    if (e >= n) return;                                       // (whole quads leave: the exchanges stay inside a quad)
    quad::x25519_element<BASE9>(out, pk, sk, e);
}

// ---- many secrets, ONE peer key: the peer's wide comb (x25519_peer.cuh) ---------------------------------------------------
// The peer's comb, the point it was built for and the key it belongs to live in a buffer of the calling thread that outlives
// the call (ThreadState::keep, slot KEEP_PEER): PEER_KEEP_WORDS words, laid out as below.  `remembered` is the peer key the
// comb was built for and a state word (0: nothing yet, 2: remembered and eligible), then the last key refused and a word that
// says whether there is one: an ineligible peer does not evict the comb of the last eligible one, and a call that repeats it
// does not pay for its Q again.  `flags` is THIS call's verdict: [0] the comb decides the call,
// [1] the call builds the comb for a new peer.  Every one-peer kernel of a call reads these words on the device: the host
// never learns the verdict, and the call does not synchronise.
constexpr size_t PEER_Q_OFFSET = WB_TBL_WORDS;
constexpr size_t PEER_REMEMBERED_OFFSET = PEER_Q_OFFSET + PEER_Q_WORDS;          // 8 key words + the state word, 8 + 1 refused
constexpr size_t PEER_FLAGS_OFFSET = PEER_REMEMBERED_OFFSET + 18;                // 2 words
constexpr size_t PEER_KEEP_WORDS = PEER_FLAGS_OFFSET + 2;
constexpr int PEER_ROW_BLOCK = 128;

// One lane: is `pk` the remembered peer?  Then the comb decides iff it was built (state 2).  The last refused key: the ladder.
// Otherwise, with build_if_new, Q = 8P and the peer's eligibility (x25519_peer_point); an eligible new peer gets Q written for
// k_x25519_peer_prepare and the remembered state cleared until k_x25519_peer_remember writes the new key down.  Without build_if_new (a call below the
// ONE_PEER_WIDE size) a new peer runs the ladder: building a comb would cost more than the call takes.
__global__ void __launch_bounds__(64) k_x25519_peer_check(u32* q_words, u32* remembered, u32* flags, const u32* __restrict__ pk,
                                                          int build_if_new)
{
    if (threadIdx.x != 0) return;
    u32 u[8], same = remembered[8] != 0, refused = remembered[17] != 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        u[j] = pk[j];
        same &= remembered[j] == u[j] ? 1u : 0u;
        refused &= remembered[9 + j] == u[j] ? 1u : 0u;
    }
    if (same) {
        flags[0] = remembered[8] == 2 ? 1u : 0u;
        flags[1] = 0;
        return;
    }
    if (!build_if_new || refused) {
        flags[0] = flags[1] = 0;
        return;
    }
    u32 q[3][8];
    const u32 ok = x25519_peer_point(q, u) ? 1u : 0u;
    if (ok) {
#pragma unroll
        for (int f = 0; f < 3; f++)
#pragma unroll
            for (int j = 0; j < 8; j++) q_words[8 * f + j] = q[f][j];
        remembered[8] = 0;                                    // the comb is about to change: no call may trust it until remembered
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++) remembered[9 + j] = u[j];
        remembered[17] = 1;
    }
    flags[0] = flags[1] = ok;
}

// the peer's comb: one packed row per thread, the work of k_gen_wide_table for Q instead of B (a call that builds nothing leaves)
__global__ void __launch_bounds__(PEER_ROW_BLOCK) k_x25519_peer_prepare(u32* wide_peer /*[WB_NT][WB_ROWS][WB_ROW_WORDS]*/,
                                                                       const u32* __restrict__ q_words, const u32* __restrict__ flags)
{
    if (!flags[1]) return;
    const u32 g = blockIdx.x * PEER_ROW_BLOCK + threadIdx.x;  // table * WB_ROWS + row
    const int table = (int)(g / WB_ROWS);
    ge_pa Q;
    x25519_peer_pa(Q, q_words);
    u32 rows[3][8];
    ge_signed_comb_row_of(rows, Q, g % WB_ROWS, (WB_NT - 1 - table) * WB_STEP, WB_TEETH, WB_COLS);
    uint4* out = reinterpret_cast<uint4*>(wide_peer + (size_t)g * WB_ROW_WORDS);
#pragma unroll
    for (int f = 0; f < 3; f++) {
        out[2 * f] = make_uint4(rows[f][0], rows[f][1], rows[f][2], rows[f][3]);
        out[2 * f + 1] = make_uint4(rows[f][4], rows[f][5], rows[f][6], rows[f][7]);
    }
    out[6] = make_uint4(2, 0, 0, 0);                          // 2Z, as in k_gen_wide_table
    out[7] = make_uint4(0, 0, 0, 0);
}

// behind the rows on the stream: the comb now belongs to `pk`
__global__ void __launch_bounds__(64) k_x25519_peer_remember(u32* remembered, const u32* __restrict__ pk, const u32* __restrict__ flags)
{
    if (threadIdx.x != 0 || !flags[1]) return;
#pragma unroll
    for (int j = 0; j < 8; j++) remembered[j] = pk[j];
    remembered[8] = 2;
}

// the walk: k_x25519_public_fast_mult<true> over the peer's comb with k >> 3; numerator and denominator to the X25519 scratch
// slots, for the shared inversion behind it
__global__ void __launch_bounds__(WB_BLOCK, 4) k_x25519_one_peer_mult(ProjScratch scr, void* sk, size_t n, const u32* __restrict__ wide_peer,
                                                                      const u32* __restrict__ flags)
{
    if (!flags[0]) return;                                    // the ladder decides this call
    __shared__ unsigned short cols[WB_COLS * WB_BLOCK];
    const size_t i = (size_t)blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
    load32(k, sk, i);
    clamp_words(k);
    store32(sk, i, k);                                        // the reference clamps in the caller's buffer
    fe num, den;
    x25519_one_peer_lane(num, den, k, wide_peer, cols + threadIdx.x, WB_BLOCK);
    soa_store_fe(scr.a, n, i, num);
    soa_store_fe(scr.z, n, i, den);
}

// ... and the ladder of the same call, the peer key read with stride 0: k_x25519_ladder for a call that does not walk the comb
// (wide_ok null: the host knows already, no comb asked for)
__global__ void __launch_bounds__(XL_BLOCK, C25519_XF_WAVES) k_x25519_ladder_one_peer(u32* X, u32* Z, const void* pk, void* sk, size_t n,
                                                                                     const u32* __restrict__ wide_ok)
{
    if (wide_ok && *wide_ok) return;                          // the comb decides this call
    const size_t i = (size_t)blockIdx.x * XL_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 u[8], k[8];
    load32(u, pk, 0);
    load32(k, sk, i);
    clamp_words(k);
    store32(sk, i, k);
    fe PX, PZ;
    x25519_ladder_xz<false>(PX, PZ, u, k);
    soa_store_fe(X, n, i, PX);
    soa_store_fe(Z, n, i, PZ);
}

// ... on quads (k_x25519_quad), for the sizes x25519_dev runs there
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) k_x25519_quad_one_peer(void* out, const void* pk, void* sk, size_t n,
                                                                                                    const u32* __restrict__ wide_ok)
{
    if (wide_ok && *wide_ok) return;
    const size_t e = (size_t)blockIdx.x * quad::ELEMS_PER_WAVE + (threadIdx.x >> 2);
    if (e >= n) return;
    quad::x25519_element<false, true>(out, pk, sk, e);
}

// the peer key as n records, for the per-wave kernels of a call that asks for no comb
__global__ void __launch_bounds__(256) k_x25519_peer_broadcast(uint4* dst, const uint4* __restrict__ pk, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * n) dst[i] = pk[i & 1];
}

// the shared inversion of a call whose ladder (on quads) wrote its results itself: it runs only where the comb decided
struct FinishX25519IfWide {
    FinishX25519 fin; const u32* wide_ok;
    C25519_DEV bool skip() const { return !*wide_ok; }
    C25519_DEV void emit(size_t e, const fe& zinv) const { fin.emit(e, zinv); }
};

// ---- many secrets, MANY peer keys: element i against context ctx_index[i] (x25519_peer_ctx.cuh) -----------------------------
// curve25519_dh_Peer_Init: one lane per key, its projective rows in lane-private scratch (QTableLimbs) until they are normalised
__global__ void __launch_bounds__(ED_BLOCK, C25519_VI_WAVES) k_x25519_peer_init(u32* ctxs, const void* pk, size_t n, u32* tables)
{
    const size_t i = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 u[8];
    load32(u, pk, i);
    peer_ctx_build(ctxs + i * PEER_CTX_WORDS, u, tables + i * QTABLE_LIMB_WORDS);
}

// the walk over the element's own context rows, read in place; numerator and denominator to the X25519 scratch slots.  An
// element whose context is not eligible goes on the ladder list (k_x25519_peer_indexed_ladder); an index >= n_ctx leaves
// num = den = 0, which the shared inversion turns into 32 zero bytes -- the ladder's answer for the key 0.
__global__ void __launch_bounds__(WB_BLOCK, 4) k_x25519_peer_indexed_walk(ProjScratch scr, void* sk, const u32* __restrict__ ctxs,
                                                                          size_t n_ctx, const u32* __restrict__ ctx_index, size_t n,
                                                                          u32* ladder_list, u32* ladder_count)
{
    __shared__ u32 cols[8 * WB_BLOCK];                        // the lane's 64 columns (peer_ctx_columns)
    const size_t i = (size_t)blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 k[8];
    load32(k, sk, i);
    clamp_words(k);
    store32(sk, i, k);                                        // the reference clamps in the caller's buffer
    const u32* ctx = peer_ctx_of(ctxs, n_ctx, ctx_index, i);
    fe num, den;
    if (ctx && ctx[PEER_CTX_ELIGIBLE] != 1u) {                // (public: which peer, and whether it lies on the curve)
        ladder_list[atomicAdd(ladder_count, 1u)] = (u32)i;
        return;
    }
    if (ctx) {
        peer_ctx_columns(cols + threadIdx.x, WB_BLOCK, k);
        peer_ctx_walk(num, den, cols + threadIdx.x, WB_BLOCK, ctx + PEER_CTX_ROWS);
    } else {
        fe_set_u32(num, 0);
        fe_set_u32(den, 0);
    }
    soa_store_fe(scr.a, n, i, num);
    soa_store_fe(scr.z, n, i, den);
}

// ... then the ladder for the listed elements, on the key their context holds, into the same scratch slots (the k_ed25519_verify_slow
// pattern: the grid covers every element, workgroups beyond the list's end read the counter and leave).  report: the list's length
// for c25519_amd_x25519_indexed_last_ladder_elements.
__global__ void __launch_bounds__(XL_BLOCK, C25519_XF_WAVES) k_x25519_peer_indexed_ladder(ProjScratch scr, const void* sk, const u32* __restrict__ ctxs,
                                                                                         const u32* __restrict__ ctx_index, size_t n,
                                                                                         const u32* __restrict__ ladder_list,
                                                                                         const u32* __restrict__ ladder_count, u32* report)
{
    const u32 count = *ladder_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) *report = count;
    const size_t j = (size_t)blockIdx.x * XL_BLOCK + threadIdx.x;
    if (j >= count) return;
    const size_t i = ladder_list[j];
    u32 u[8], k[8];
    peer_ctx_key(u, ctxs + (size_t)ctx_index[i] * PEER_CTX_WORDS);    // (listed: the index is in range)
    load32(k, sk, i);                                         // (clamped by the walk kernel)
    fe PX, PZ;
    x25519_ladder_xz<false>(PX, PZ, u, k);
    soa_store_fe(scr.a, n, i, PX);
    soa_store_fe(scr.z, n, i, PZ);
}

// the key of each element's context as n records (32 zero bytes for an index >= n_ctx), for a call that runs what
// curve25519_dh_CreateSharedKey_dev runs: one 16-byte half per thread
__global__ void __launch_bounds__(256) k_x25519_peer_gather(uint4* keys, const u32* __restrict__ ctxs, size_t n_ctx,
                                                            const u32* __restrict__ ctx_index, size_t n)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= 2 * n) return;
    const u32* ctx = peer_ctx_of(ctxs, n_ctx, ctx_index, g >> 1);
    keys[g] = ctx ? reinterpret_cast<const uint4*>(ctx)[g & 1] : make_uint4(0, 0, 0, 0);
}

namespace {

// lanes per X25519 workgroup for a batch of n: the widest shape that still puts a wave on every SIMD the batch can reach
// (256 CUs x 4 SIMDs; 2^16 elements are 1024 waves).  profiles/r03_batch_sweep.txt has both shapes side by side.
int x25519_block_for(size_t n)
{
    n = std::max(n, c25519_host::batch_shape_hint());         // a piece of a pipelined *_batch call: the whole call counts
    if (n <= ((size_t)1 << 16)) return 64;
    if (n <= ((size_t)1 << 17)) return 128;
    if (n <= ((size_t)1 << 18)) return 256;
    return XF_BLOCK;
}
// a batch that fills the chip runs the ladder and the shared inversion as two launches (k_x25519_ladder's comment);
// tunable XF_SPLIT = 0 / 1 forces either shape (A/B knob)
bool x25519_split_for(size_t n)
{
    const long v = c25519_host::tunable(c25519_host::T_XF_SPLIT);
    if (v != c25519_host::T_UNSET) return v != 0;
    return std::max(n, c25519_host::batch_shape_hint()) > ((size_t)1 << 16);   // measured at the sustained clock: two launches win from 2^17 up (3 / 2 / 1.2 % at 2^17 / 2^18 / 2^20), one launch by 1 % below
}
template <int BLOCK>
void x25519_launch(void* out, const void* pk, void* sk, size_t n, hipStream_t stream)
{
    if (pk) k_x25519_fused<false, BLOCK><<<grid_for(n, BLOCK), BLOCK, 0, stream>>>(out, pk, sk, n);
    else    k_x25519_fused<true, BLOCK><<<grid_for(n, BLOCK), BLOCK, 0, stream>>>(out, pk, sk, n);
}

}  // namespace

extern "C" {

#ifdef C25519_CYCLE_PROBE
// measurement builds only: where the waves of k_x25519_fused write their stamps (PROBE_WORDS u64 per wave), or null
int c25519_amd_probe_set(void* buf)
{
    C25519_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_cycle_probe), &buf, sizeof buf));
    return 0;
}
int c25519_amd_probe_words(void) { return PROBE_WORDS; }
#endif

// ---- device-pointer entry points ----------------------------------------------------------------

// work: null, or the projective part's scratch (Carve::proj(n)) the caller holds already on this stream, in a lease of its own
static int x25519_dev(void* out, const void* pk, void* sk, size_t n, hipStream_t stream, u32* work = nullptr)
{
    if (x25519_quad_for(n)) {                                 // four lanes per element
        const unsigned grid = grid_for(n, quad::ELEMS_PER_WAVE);
        note_shape(SHAPE_QUAD, 64);
        if (pk) k_x25519_quad<false><<<grid, 64, 0, stream>>>(out, pk, sk, n);
        else    k_x25519_quad<true><<<grid, 64, 0, stream>>>(out, pk, sk, n);
        C25519_TRY(hipGetLastError());
        return 0;
    }
    if (x25519_coop_for(n)) {
        const CallWords cw = call_words(n, pk, sk);
        const bool two_waves = pk && x25519_two_waves_for(n);
        note_shape(SHAPE_PER_GROUP, two_waves ? 128 : 64);
        if (two_waves) k_x25519_coop2<<<(unsigned)n, 128, 0, stream>>>(out, pk, sk, n, take_done_word(n), cw);
        else if (pk) k_x25519_coop<false><<<(unsigned)n, 64, 0, stream>>>(out, pk, sk, n, take_done_word(n), cw);
        else    k_x25519_coop<true><<<(unsigned)n, 64, 0, stream>>>(out, pk, sk, n, take_done_word(n), cw);
        C25519_TRY(hipGetLastError());
        return 0;
    }
    if (x25519_split_for(n)) {
        ProjScratch scr;
        c25519_host::WorkLease lease;
        C25519_RC(lease_proj(&scr, lease, n, stream, work));
        note_shape(SHAPE_LANE_INVERT, XL_BLOCK);
        if (pk) k_x25519_ladder<false><<<grid_for(n, XL_BLOCK), XL_BLOCK, 0, stream>>>(scr.a, scr.z, pk, sk, n);
        else    k_x25519_ladder<true><<<grid_for(n, XL_BLOCK), XL_BLOCK, 0, stream>>>(scr.a, scr.z, pk, sk, n);
        C25519_TRY(hipGetLastError());
        C25519_RC(launch_invert(scr, n, FinishX25519{ scr.a, out, n }, stream));
        return lease.release();
    }
    const int block = x25519_block_for(n);
    note_shape(SHAPE_LANE, block);
    switch (block) {
    case 64:  x25519_launch<64>(out, pk, sk, n, stream); break;
    case 128: x25519_launch<128>(out, pk, sk, n, stream); break;
    case 256: x25519_launch<256>(out, pk, sk, n, stream); break;
    default:  x25519_launch<XF_BLOCK>(out, pk, sk, n, stream); break;
    }
    C25519_TRY(hipGetLastError());
    return 0;
}

int curve25519_dh_CreateSharedKey_dev(void* shared, const void* pk, void* sk, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!shared || !pk || !sk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { shared, pk, sk })) return rc;
    if (n == 0) return 0;
    return x25519_dev(shared, pk, sk, n, (hipStream_t)stream);
}

int curve25519_dh_CalculatePublicKey_dev(void* pk, void* sk, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!pk || !sk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { pk, sk })) return rc;
    if (n == 0) return 0;
    return x25519_dev(pk, nullptr, sk, n, (hipStream_t)stream);
}

// ---- many secrets, one peer key ----------------------------------------------------------------

// the smallest call that builds a comb for a NEW peer (tunable ONE_PEER_WIDE; 0 = never).  A call that builds one takes 0.75 ms
// plus the walk (~1.3 G/s): it loses to the ladder at 2^16 (0.75 against 0.68 ms) and wins at 3 * 2^15 (0.80 against 1.11 ms)
// and above (tools/one_peer_rate.py, profiles/one_peer_rate.txt).
constexpr long ONE_PEER_WIDE_DEFAULT = 3L << 15;

// what the calling thread's last one-peer call on this device left behind for c25519_amd_x25519_one_peer_last_wide: where its
// 0 (the call never asked the device), or where its "the comb decides this call" word lives
static thread_local c25519_host::LastCall tl_last_peer;

// Above the per-wave range a thread that has kept a peer comb asks the device, at any size, whether this call's key is that peer
// (one lane, 72 bytes); from ONE_PEER_WIDE elements on (the whole of a pipelined *_batch call counts) a new eligible peer gets
// its comb built first.  The comb walk and the ladder are both enqueued, each kernel leaves at once when the device's verdict
// is the other's; the ladder is the kernel x25519_dev runs at this size -- on quads, or one lane per element (split from the
// shared inversion, which both feed).  A call that asks nothing runs the ladder with stride-0 keys, or -- per-wave sizes -- the
// per-wave kernels on the key broadcast to n records.
static int x25519_one_peer_dev(void* out, const void* pk, void* sk, size_t n, hipStream_t stream)
{
    using c25519_host::ThreadState;
    const long wide_from = c25519_host::tunable_or(c25519_host::T_ONE_PEER_WIDE, ONE_PEER_WIDE_DEFAULT);   // (read once per call)
    const size_t whole = std::max(n, c25519_host::batch_shape_hint());
    const bool quads = x25519_quad_for(n);
    const bool per_wave = !quads && x25519_coop_for(n);
    const bool build = wide_from > 0 && whole >= (size_t)wide_from;
    const bool reuse = !build && wide_from > 0 && !per_wave && tls().has_keep(ThreadState::KEEP_PEER);
    tl_last_peer = c25519_host::LastCall::known(0);
    if (!build && !reuse && per_wave) {                      // a few elements: one (or two) waves per element, as x25519_dev runs them
        c25519_host::WorkLease lease;
        const void* keys = pk;
        if (n > 1) {
            u32* copies = nullptr;                            // the key, n times
            C25519_RC(lease_scratch(&copies, lease, stream, [n](Carve& c) { return c.take(8 * n); }));
            k_x25519_peer_broadcast<<<grid_for(2 * n, 256), 256, 0, stream>>>((uint4*)copies, (const uint4*)pk, n);
            C25519_TRY(hipGetLastError());
            keys = copies;
        }
        const CallWords cw{};                                 // (records from memory: pk is device memory even in a zero-copy call)
        if (x25519_two_waves_for(n)) k_x25519_coop2<<<(unsigned)n, 128, 0, stream>>>(out, keys, sk, n, take_done_word(n), cw);
        else k_x25519_coop<false><<<(unsigned)n, 64, 0, stream>>>(out, keys, sk, n, take_done_word(n), cw);
        C25519_TRY(hipGetLastError());
        return lease.release();
    }
    ProjScratch scr;
    c25519_host::WorkLease lease;
    const bool scratch = build || reuse || !quads;           // (the quads' ladder writes its results itself: 256 bytes nobody uses)
    C25519_RC(lease_scratch(&scr, lease, stream, [=](Carve& c) {
        if (scratch) return c.proj(n);
        c.take(64);
        return ProjScratch{};
    }));
    const u32* wide_ok = nullptr;
    c25519_host::KeepLease keep_lease;                        // records the kept buffer's event however this call leaves
    if (build || reuse) {
        void* keep = nullptr;
        bool fresh = false;
        C25519_RC(keep_lease.acquire(&keep, PEER_KEEP_WORDS * sizeof(u32), stream, &fresh, ThreadState::KEEP_PEER));
        u32* wide_peer = (u32*)keep;
        u32* flags = wide_peer + PEER_FLAGS_OFFSET;
        wide_ok = flags;
        k_x25519_peer_check<<<1, 64, 0, stream>>>(wide_peer + PEER_Q_OFFSET, wide_peer + PEER_REMEMBERED_OFFSET, flags, (const u32*)pk,
                                                  build ? 1 : 0);
        C25519_TRY(hipGetLastError());
        if (build) {
            k_x25519_peer_prepare<<<WB_NT * WB_ROWS / PEER_ROW_BLOCK, PEER_ROW_BLOCK, 0, stream>>>(wide_peer, wide_peer + PEER_Q_OFFSET, flags);
            C25519_TRY(hipGetLastError());
            k_x25519_peer_remember<<<1, 64, 0, stream>>>(wide_peer + PEER_REMEMBERED_OFFSET, (const u32*)pk, flags);
            C25519_TRY(hipGetLastError());
        }
        k_x25519_one_peer_mult<<<grid_for(n, WB_BLOCK), WB_BLOCK, 0, stream>>>(scr, sk, n, wide_peer, flags);
        C25519_TRY(hipGetLastError());
        tl_last_peer.reports_in(wide_ok, stream);
    }
    if (quads) {
        k_x25519_quad_one_peer<<<grid_for(n, quad::ELEMS_PER_WAVE), 64, 0, stream>>>(out, pk, sk, n, wide_ok);
        C25519_TRY(hipGetLastError());
        if (wide_ok) C25519_RC(launch_invert(scr, n, FinishX25519IfWide{ FinishX25519{ scr.a, out, n }, wide_ok }, stream));
    } else {
        k_x25519_ladder_one_peer<<<grid_for(n, XL_BLOCK), XL_BLOCK, 0, stream>>>(scr.a, scr.z, pk, sk, n, wide_ok);
        C25519_TRY(hipGetLastError());
        C25519_RC(launch_invert(scr, n, FinishX25519{ scr.a, out, n }, stream));
    }
    C25519_RC(keep_lease.release());
    return lease.release();
}

int curve25519_dh_CreateSharedKey_one_peer_dev(void* shared, const void* pk, void* sk, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!shared || !pk || !sk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { shared, pk, sk })) return rc;
    if (n == 0) return 0;
    return x25519_one_peer_dev(shared, pk, sk, n, (hipStream_t)stream);
}

// test / accounting hook: did the calling thread's last one-peer call on this device walk the peer's comb (1), or the ladder (0: the
// call did not ask -- per-wave size, no kept comb below ONE_PEER_WIDE, ONE_PEER_WIDE = 0 -- or the device said no: another peer
// than the remembered one below ONE_PEER_WIDE, a peer off the curve or u = -1)?  -1: no such call.  Synchronises with that call's
// stream.  (A *_batch call of several pieces reports its last piece.)
long c25519_amd_x25519_one_peer_last_wide(void)
{
    C25519_API_CALL_OR(-1);
    const long v = tl_last_peer.read();
    return v > 0 ? 1 : v;
}

// ---- many secrets, many peer contexts -------------------------------------------------------------------------

// keys per k_x25519_peer_init launch: bounds its lane-private scratch (2.5 KiB per key) at 80 MiB
constexpr size_t PEER_INIT_CHUNK = (size_t)1 << 15;

int curve25519_dh_Peer_Init_dev(void* ctx, const void* pk, size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!ctx || !pk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { ctx, pk })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t chunk = std::min(n, PEER_INIT_CHUNK);
    u32* w = nullptr;                                         // a launch's lane-private tables
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&w, lease, stream, [chunk](Carve& c) { return c.take(chunk * QTABLE_LIMB_WORDS); }));
    for (size_t lo = 0; lo < n; lo += chunk) {
        const size_t c = std::min(chunk, n - lo);
        k_x25519_peer_init<<<grid_for(c, ED_BLOCK), ED_BLOCK, 0, stream>>>((u32*)ctx + lo * PEER_CTX_WORDS, (const uint4*)pk + 2 * lo, c,
                                                                             w);
        C25519_TRY(hipGetLastError());
    }
    return lease.release();
}

// the smallest call that walks the contexts' rows (tunable PEER_INDEXED_MIN; 0 = always).  Up to 2^16 secrets a call of the walk takes
// one lane's latency, 0.27 ms whatever its size; the per-wave ladder finishes sooner up to 2048 secrets (0.14-0.24 ms) and later from
// 2304 on (0.28 ms), so a smaller call gathers the keys and runs what curve25519_dh_CreateSharedKey_dev runs at its size
// (tools/peer_indexed_rate.py, profiles/peer_indexed_rate.txt).
constexpr long PEER_INDEXED_MIN_DEFAULT = 2049;

// what the calling thread's last indexed call on this device left behind for c25519_amd_x25519_indexed_last_ladder_elements: the
// elements the host knows ran the ladder (the whole call below PEER_INDEXED_MIN), or the device word the ladder kernel reports in
static thread_local c25519_host::LastCall tl_last_indexed;

static int x25519_indexed_dev(void* out, const void* ctxs, size_t n_ctx, const void* ctx_index, void* sk, size_t n, hipStream_t stream)
{
    const long min_walk = c25519_host::tunable_or(c25519_host::T_PEER_INDEXED_MIN, PEER_INDEXED_MIN_DEFAULT);
    const size_t whole = std::max(n, c25519_host::batch_shape_hint());
    tl_last_indexed = c25519_host::LastCall();
    c25519_host::WorkLease lease;
    if (whole < (size_t)std::max(min_walk, 0L)) {
        const bool split = !x25519_quad_for(n) && !x25519_coop_for(n) && x25519_split_for(n);
        struct Gathered { u32 *keys, *work; } g;
        C25519_RC(lease_scratch(&g, lease, stream, [=](Carve& c) {
            Gathered s;
            s.keys = c.take4(8 * n);
            s.work = split ? c.proj(n).a : nullptr;          // x25519_dev's scratch where it runs ladder and inversion in two launches
            return s;
        }));
        k_x25519_peer_gather<<<grid_for(2 * n, 256), 256, 0, stream>>>((uint4*)g.keys, (const u32*)ctxs, n_ctx, (const u32*)ctx_index, n);
        C25519_TRY(hipGetLastError());
        bool& zero_copy = c25519_host::zero_copy_call();      // the gathered keys are device memory, not the call's host records
        const bool zc = zero_copy;
        zero_copy = false;
        const int rc = x25519_dev(out, g.keys, sk, n, stream, g.work);
        zero_copy = zc;
        C25519_RC(rc);
        tl_last_indexed = c25519_host::LastCall::known((long)n);
        return lease.release();
    }
    unsigned* report = nullptr;
    C25519_RC(tls().report_word_for(&report, c25519_host::REPORT_LADDER_ELEMENTS, stream));
    struct WalkScratch { ProjScratch scr; u32 *list, *count; } ws;
    C25519_RC(lease_scratch(&ws, lease, stream, [n](Carve& c) {
        WalkScratch s;
        s.scr = c.proj(n);
        s.list = c.take4(n);                                 // the elements the ladder has to run ...
        s.count = c.take(4);                                 // ... and how many: one word used
        return s;
    }));
    const auto& [scr, list, count] = ws;
    C25519_TRY(hipMemsetAsync(count, 0, sizeof(u32), stream));
    k_x25519_peer_indexed_walk<<<grid_for(n, WB_BLOCK), WB_BLOCK, 0, stream>>>(scr, sk, (const u32*)ctxs, n_ctx, (const u32*)ctx_index, n,
                                                                              list, count);
    C25519_TRY(hipGetLastError());
    k_x25519_peer_indexed_ladder<<<grid_for(n, XL_BLOCK), XL_BLOCK, 0, stream>>>(scr, sk, (const u32*)ctxs, (const u32*)ctx_index, n,
                                                                                list, count, report);
    C25519_TRY(hipGetLastError());
    C25519_RC(launch_invert(scr, n, FinishX25519{ scr.a, out, n }, stream));
    tl_last_indexed.reports_in(report, stream);
    return lease.release();
}

int curve25519_dh_CreateSharedKey_indexed_dev(void* shared, const void* ctxs, size_t n_ctx, const void* ctx_index, void* sk, size_t n,
                                              void* stream)
{
    C25519_API_CALL();
    if (!shared || !ctxs || !ctx_index || !sk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { shared, ctxs, ctx_index, sk })) return rc;
    if (n == 0) return 0;
    if (n_ctx == 0) return bad_arg("no contexts");
    return x25519_indexed_dev(shared, ctxs, n_ctx, ctx_index, sk, n, (hipStream_t)stream);
}

// test / accounting hook: how many elements of the calling thread's last indexed call on this device ran the ladder -- all of them
// below PEER_INDEXED_MIN, otherwise those whose context is not eligible.  -1: no such call.  Synchronises with that call's stream.
// (A *_batch call of several pieces reports its last piece.)
long c25519_amd_x25519_indexed_last_ladder_elements(void)
{
    C25519_API_CALL_OR(-1);
    return tl_last_indexed.read();
}

}  // extern "C"
