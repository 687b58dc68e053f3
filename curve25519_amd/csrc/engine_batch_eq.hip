// curve25519_amd/csrc/engine_batch_eq.hip -- ed25519_VerifyBatch_zip215_*: ONE equation per call under the ZIP-215 rule (a random
// linear combination of the n cofactored equations, include/curve25519_amd.h), as a bucket-method multi-scalar multiplication over
// the 2n decoded points -- kernels, the *_dev entry points and the host-pointer forms
// (one of the engine's translation units: engine_common.cuh says which is which; the lane-level code: msm25519.cuh)
#include "engine_common.cuh"
#include "msm25519.cuh"
#include "msm_stages.cuh"

#include <cerrno>
#include <sys/random.h>

// (BatchEqScratch, the scratch of one equation as the kernels take it, and BatchEqShape: msm_stages.cuh)
struct BatchEqSeed { u32 w[8]; };

constexpr int BE_BLOCK = 256;
constexpr int BE_MAX_BUCKETS = 1 << (MSM_C_MAX - 1);

// stage 2 (it runs first: the scalar lanes leave a rejected element's s_i out): one lane per point
__global__ void __launch_bounds__(ED_BLOCK, 3) k_ed25519_batcheq_points(BatchEqScratch s, const void* sig, const void* pk, size_t n)
{
    const size_t j = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (j >= 2 * n) return;
    const bool is_r = j >= n;
    const size_t e = is_r ? j - n : j;
    u32 w[8], row[24];
    if (is_r) load32(w, sig, 2 * e); else load32(w, pk, e);
    const u32 ok = msm_point_row(row, w);
    uint4* out = reinterpret_cast<uint4*>(s.rows + j * MSM_ROW_WORDS);
#pragma unroll
    for (int g = 0; g < 6; g++) out[g] = make_uint4(row[4 * g], row[4 * g + 1], row[4 * g + 2], row[4 * g + 3]);
    if (!ok) { atomicOr(&s.flags[e], 1u); atomicOr(s.reject, 1u); }
}

// stage 1: one lane per element; the workgroup's sum of the s_i leaves as 16 chunk sums (one wave-wide reduction, then one LDS atomic
// per wave and chunk)
__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_batcheq_scalars(BatchEqScratch s, const void* sig, const void* pk, Msgs msgs, size_t n,
                                                                      BatchEqSeed seed, unsigned long long index0, BatchEqShape shape)
{
    __shared__ u32 part[16];
    if (threadIdx.x < 16) part[threadIdx.x] = 0;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * BE_BLOCK + threadIdx.x;
    u32 sv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (i < n) {
        u32 pkw[8], Rw[8], Sw[8], a[8], z[8];
        load32(pkw, pk, i);
        load32(Rw, sig, 2 * i);
        load32(Sw, sig, 2 * i + 1);
        const u32 s_ok = msm_scalars(a, z, sv, pkw, Rw, Sw, msgs.ptr(i), msgs.len(i), seed.w, index0 + i, shape.c);
        soa_store8(s.sc, 2 * n, i, a);
        soa_store8(s.sc, 2 * n, n + i, z);
        if (!s_ok) { s.flags[i] = 1u; atomicOr(s.reject, 1u); }
        if (!s_ok || s.flags[i]) {
#pragma unroll
            for (int j = 0; j < 8; j++) sv[j] = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
        u32 v = (sv[j >> 1] >> (16 * (j & 1))) & 0xffffu;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) atomicAdd(&part[j], v);
    }
    __syncthreads();
    if (threadIdx.x < 16) s.partial[(size_t)blockIdx.x * 16 + threadIdx.x] = part[threadIdx.x];
}

// stage 3, twice: blockIdx.y = window, blockIdx.x = a run of `pts` points.  The workgroup counts its points' digits per bucket in LDS,
// then touches each global counter it needs ONCE: to add its count (count pass), or to reserve that many slots of the bucket's list
// (scatter pass), which its lanes then fill in whatever order the LDS atomics hand out.
// Points 0 .. nk - 1 are keys, nk .. N - 1 the R's; the flag of R point p is flags[p - rflag] (rflag = n where key i and R i share
// element i's flag, 0 where every point has a flag of its own: the coalesced equation).
template <bool Scatter>
C25519_DEV void batcheq_digits(const BatchEqScratch& s, size_t nk, size_t N, size_t rflag, unsigned pts, const BatchEqShape& shape, u32* hist,
                               u32* base)
{
    const int w = blockIdx.y;
    const size_t p0 = (size_t)blockIdx.x * pts, p1 = p0 + pts < N ? p0 + pts : N;
    if (p0 >= nk ? msm_window_digit(shape, w, true) < 0 : (p1 <= nk && w == shape.wa)) return;   // (uniform) no point of this run has a digit here
    for (int b = threadIdx.x; b < shape.buckets; b += BE_BLOCK) hist[b] = 0;
    __syncthreads();
    auto digit_of = [&](size_t p) -> int {
        const bool is_r = p >= nk;
        const int dw = msm_window_digit(shape, w, is_r);
        if (dw < 0 || s.flags[is_r ? p - rflag : p]) return 0;
        return msm_digit(s.sc + p, N, dw, shape.c, is_r ? shape.wz : shape.wa);
    };
    for (size_t p = p0 + threadIdx.x; p < p1; p += BE_BLOCK) {
        const int d = digit_of(p);
        if (d) atomicAdd(&hist[msm_slot(shape, w, d < 0 ? -d : d, (u32)p)], 1u);
    }
    __syncthreads();
    u32* global = (Scatter ? s.cursor : s.counts) + (size_t)w * shape.buckets;
    for (int b = threadIdx.x; b < shape.buckets; b += BE_BLOCK) {
        const u32 cnt = hist[b];
        if (!cnt) continue;
        const u32 at = atomicAdd(&global[b], cnt);
        if (Scatter) { base[b] = at; hist[b] = 0; }
    }
    if (!Scatter) return;
    __syncthreads();
    for (size_t p = p0 + threadIdx.x; p < p1; p += BE_BLOCK) {
        const int d = digit_of(p);
        if (!d) continue;
        const u32 b = msm_slot(shape, w, d < 0 ? -d : d, (u32)p);
        s.entries[base[b] + atomicAdd(&hist[b], 1u)] = ((u32)p << 1) | (d < 0 ? 1u : 0u);
    }
}

__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_batcheq_count(BatchEqScratch s, size_t n, unsigned pts, BatchEqShape shape)
{
    __shared__ u32 hist[BE_MAX_BUCKETS];
    batcheq_digits<false>(s, n, 2 * n, n, pts, shape, hist, nullptr);
}

__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_batcheq_scatter(BatchEqScratch s, size_t n, unsigned pts, BatchEqShape shape)
{
    __shared__ u32 hist[BE_MAX_BUCKETS], base[BE_MAX_BUCKETS];
    batcheq_digits<true>(s, n, 2 * n, n, pts, shape, hist, base);
}

// exclusive scan of the K counts into cursor: one workgroup, a run of counters per lane
constexpr int BE_SCAN_BLOCK = 1024;
__global__ void __launch_bounds__(BE_SCAN_BLOCK) k_ed25519_batcheq_scan(BatchEqScratch s, unsigned K)
{
    __shared__ u32 sums[BE_SCAN_BLOCK];
    const unsigned per = (K + BE_SCAN_BLOCK - 1) / BE_SCAN_BLOCK, lo = threadIdx.x * per, hi = lo + per < K ? lo + per : K;
    u32 mine = 0;
    for (unsigned k = lo; k < hi; k++) mine += s.counts[k];
    sums[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < BE_SCAN_BLOCK; o <<= 1) {
        const u32 v = (int)threadIdx.x >= o ? sums[threadIdx.x - o] : 0u;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    u32 at = sums[threadIdx.x] - mine;
    for (unsigned k = lo; k < hi; k++) {
        s.cursor[k] = at;
        at += s.counts[k];
    }
}

// stage 4: one lane per (window, bucket)
__global__ void __launch_bounds__(ED_BLOCK, 2) k_ed25519_batcheq_buckets(BatchEqScratch s, unsigned K)
{
    const unsigned k = blockIdx.x * ED_BLOCK + threadIdx.x;
    if (k >= K) return;
    const u32 end = s.cursor[k], begin = end - s.counts[k];
    ge_ext S;
    msm_bucket_sum(S, s.rows, s.entries, begin, end);
    msm_store_ext(s.buckets + (size_t)k * MSM_EXT_WORDS, S);
}

// stage 5: one wave per window, buckets / 64 consecutive buckets per lane, then a tree over the 64 chunk sums through LDS
__global__ void __launch_bounds__(64) k_ed25519_batcheq_windows(BatchEqScratch s, BatchEqShape shape)
{
    __shared__ u32 red[MSM_EXT_WORDS * 64];
    const int w = blockIdx.x, l = threadIdx.x;
    const u32 m = (u32)shape.buckets / 64;
    ge_ext acc, t;
    msm_chunk_sum(acc, s.buckets + (size_t)w * shape.buckets * MSM_EXT_WORDS, l * m, (l + 1) * m, msm_window_rlog2(shape, w));
    const fe* f[4] = { &acc.X, &acc.Y, &acc.Z, &acc.T };
    fe* g[4] = { &t.X, &t.Y, &t.Z, &t.T };
#pragma unroll 1
    for (int o = 32; o >= 1; o >>= 1) {
        if (l >= o && l < 2 * o) {
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int i = 0; i < 10; i++) red[(10 * j + i) * 64 + l] = f[j]->v[i];
        }
        __syncthreads();
        if (l < o) {
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int i = 0; i < 10; i++) g[j]->v[i] = red[(10 * j + i) * 64 + l + o];
            msm_ext_add(acc, t);
        }
        __syncthreads();
    }
    if (l == 0) msm_store_ext(s.windows + (size_t)w * MSM_EXT_WORDS, acc);
}

// stage 6: two waves.  Wave 1 adds up the workgroups' chunk sums of the s_i and its first lane walks the wide comb with the total;
// meanwhile the first lane of wave 0 combines the windows.  Then T = both, and either enc(T) (the hook) or the verdict.
__global__ void __launch_bounds__(128) k_ed25519_batcheq_tail(BatchEqScratch s, BatchEqShape shape, unsigned blocks, const u32* __restrict__ wide,
                                                              int* result, void* point_out)
{
    __shared__ u64 sums[64];
    __shared__ __attribute__((aligned(16))) u32 sb[MSM_EXT_WORDS];
    __shared__ unsigned short cols[WB_COLS];
    const int t = threadIdx.x;
    if (t >= 64) {
        const int chunk = t & 15, q = (t - 64) >> 4;
        u64 v = 0;
        for (unsigned b = q; b < blocks; b += 4) v += s.partial[(size_t)b * 16 + chunk];
        sums[t - 64] = v;
    }
    __syncthreads();
    ge_ext T;
    if (t == 64) {
        u64 chunk[16];
#pragma unroll
        for (int j = 0; j < 16; j++) chunk[j] = sums[j] + sums[16 + j] + sums[32 + j] + sums[48 + j];
        u32 sw[8];
        msm_fold_s(sw, chunk);
        wb_columns<true>(cols, 1, sw);
        ge_ext SB;
        ge_base_mult_wide<true>(SB, wide, cols, 1);
        msm_store_ext(sb, SB);
    } else if (t == 0)
        msm_horner(T, s.windows, shape);
    __syncthreads();
    if (t != 0) return;
    ge_ext SB;
    msm_load_ext(SB, sb);
    msm_ext_add(T, SB);
    if (point_out) {
        u32 enc[8];
        msm_encode(enc, T);
        store32(point_out, 0, enc);
        return;
    }
    const u32 neutral = msm_times8_is_neutral(T);
    *result = (neutral && *s.reject == 0) ? 1 : 0;
}

// calls below BATCH_EQ_MIN: the AND of the per-element verdicts.  Every workgroup ANDs a stride of them and ORs its finding into
// state[0]; the last one to take a ticket (state[1]) writes the result.  state: two zeroed words (null: n == 0, the empty AND).
constexpr int BE_AND_BLOCK = 1024;
__global__ void __launch_bounds__(BE_AND_BLOCK) k_ed25519_batcheq_and(int* result, const int* verdict, size_t n, u32* state)
{
    int ok = 1;
    for (size_t i = (size_t)blockIdx.x * BE_AND_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BE_AND_BLOCK) ok &= verdict[i] == 1;
    ok = __syncthreads_and(ok);
    if (threadIdx.x != 0) return;
    if (!state) { *result = 1; return; }
    if (!ok) atomicOr(&state[0], 1u);
    __threadfence();
    if (atomicAdd(&state[1], 1u) == gridDim.x - 1) *result = atomicOr(&state[0], 0u) ? 0 : 1;
}

// ---- the coalesced equation (ed25519_VerifyBatch_zip215_indexed_*): n elements name K keys, N = K + n points (the keys, then the R's).
// BatchEqScratch cut for that shape (keyeq_layout): flags has one word per POINT -- a key's: it does not decode, or its scalar is
// zero; an R's: its element is left out --, and keysum holds eight 64-bit sums per key.  The scan, the buckets, the windows and the
// tail are the kernels above.

// stages 1 and 2: one lane per point.  A key that does not decode only gets its flag: whether that matters is up to who names it.
__global__ void __launch_bounds__(ED_BLOCK, 3) k_ed25519_keyeq_points(BatchEqScratch s, const void* sig, const void* keys, size_t K, size_t n)
{
    const size_t j = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (j >= K + n) return;
    const bool is_r = j >= K;
    u32 w[8], row[24];
    if (is_r) load32(w, sig, 2 * (j - K)); else load32(w, keys, j);
    const u32 ok = msm_point_row(row, w);
    uint4* out = reinterpret_cast<uint4*>(s.rows + j * MSM_ROW_WORDS);
#pragma unroll
    for (int g = 0; g < 6; g++) out[g] = make_uint4(row[4 * g], row[4 * g + 1], row[4 * g + 2], row[4 * g + 3]);
    if (!ok) {
        s.flags[j] = 1u;
        if (is_r) atomicOr(s.reject, 1u);
    }
}

// stage 3: one lane per element.  The s_i leave as in k_ed25519_batcheq_scalars.  The a_i of the elements that stay are summed per key,
// word by word, in LDS first -- an open-addressed table of the keys this workgroup met, twice as many slots as lanes -- and each slot
// in use then adds its eight sums to the key's in memory: one 64-bit atomic per workgroup, key and word, none of which returns a value.
constexpr int KE_SLOTS = 2 * BE_BLOCK;
constexpr u32 KE_EMPTY = 0xffffffffu;                        // (a key index is below 2^26)
__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_keyeq_scalars(BatchEqScratch s, unsigned long long* keysum, const void* sig, const void* keys,
                                                                    const u32* key_index, Msgs msgs, size_t n, size_t K, BatchEqSeed seed,
                                                                    unsigned long long index0, BatchEqShape shape)
{
    __shared__ u32 part[16];
    __shared__ u32 slot_key[KE_SLOTS];
    __shared__ unsigned long long slot_sum[KE_SLOTS][8];
    if (threadIdx.x < 16) part[threadIdx.x] = 0;
    for (int t = threadIdx.x; t < KE_SLOTS; t += BE_BLOCK) {
        slot_key[t] = KE_EMPTY;
#pragma unroll
        for (int j = 0; j < 8; j++) slot_sum[t][j] = 0;
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * BE_BLOCK + threadIdx.x;
    u32 sv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (i < n) {
        u32 pkw[8], Rw[8], Sw[8], a[8], z[8];
        const u32 idx = key_index[i];
        const bool in_range = idx < K;
        load32(pkw, keys, in_range ? idx : 0);               // (nothing outside keys is read)
        load32(Rw, sig, 2 * i);
        load32(Sw, sig, 2 * i + 1);
        const u32 s_ok = msm_scalars_canonical(a, z, sv, pkw, Rw, Sw, msgs.ptr(i), msgs.len(i), seed.w, index0 + i, shape.c);
        soa_store8(s.sc, K + n, K + i, z);
        if (!s_ok || !in_range || s.flags[K + i] || s.flags[idx]) {
            s.flags[K + i] = 1u;
            atomicOr(s.reject, 1u);
#pragma unroll
            for (int j = 0; j < 8; j++) sv[j] = 0;
        } else {
            u32 h = (idx * 0x9e3779b1u) >> 23;               // 9 bits: KE_SLOTS
            for (;;) {
                const u32 prev = atomicCAS(&slot_key[h], KE_EMPTY, idx);
                if (prev == KE_EMPTY || prev == idx) break;
                h = (h + 1) & (KE_SLOTS - 1);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) atomicAdd(&slot_sum[h][j], (unsigned long long)a[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
        u32 v = (sv[j >> 1] >> (16 * (j & 1))) & 0xffffu;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) atomicAdd(&part[j], v);
    }
    __syncthreads();
    if (threadIdx.x < 16) s.partial[(size_t)blockIdx.x * 16 + threadIdx.x] = part[threadIdx.x];
    for (int t = threadIdx.x; t < KE_SLOTS; t += BE_BLOCK) {
        const u32 key = slot_key[t];
        if (key == KE_EMPTY) continue;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const unsigned long long v = slot_sum[t][j];
            if (v) atomicAdd(&keysum[(size_t)key * 8 + j], v);
        }
    }
}
static_assert(KE_SLOTS == 512, "k_ed25519_keyeq_scalars hashes a key index to 9 bits");

// stage 4: one lane per key: its sums -> its one biased scalar, at the key's point
__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_keyeq_fold(BatchEqScratch s, const unsigned long long* keysum, size_t K, size_t n, BatchEqShape shape)
{
    const size_t j = (size_t)blockIdx.x * BE_BLOCK + threadIdx.x;
    if (j >= K) return;
    u64 sum[8];
#pragma unroll
    for (int w = 0; w < 8; w++) sum[w] = keysum[j * 8 + w];
    u32 a[8];
    const u32 any = msm_key_fold(a, sum, shape.c);
    soa_store8(s.sc, K + n, j, a);
    if (!any) s.flags[j] = 1u;
}

// stage 5: the digit passes with the key / R boundary at K
__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_keyeq_count(BatchEqScratch s, size_t K, size_t n, unsigned pts, BatchEqShape shape)
{
    __shared__ u32 hist[BE_MAX_BUCKETS];
    batcheq_digits<false>(s, K, K + n, 0, pts, shape, hist, nullptr);
}

__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_keyeq_scatter(BatchEqScratch s, size_t K, size_t n, unsigned pts, BatchEqShape shape)
{
    __shared__ u32 hist[BE_MAX_BUCKETS], base[BE_MAX_BUCKETS];
    batcheq_digits<true>(s, K, K + n, 0, pts, shape, hist, base);
}

// calls below BATCH_EQ_INDEXED_MIN: pk[i] = keys[key_index[i]] for the per-element kernels; an index out of range takes key 0 and
// sets the AND's finding (state[0] of k_ed25519_batcheq_and) itself
__global__ void __launch_bounds__(BE_BLOCK) k_ed25519_keyeq_gather(void* pk, const void* keys, const u32* key_index, size_t n, size_t K, u32* state)
{
    const size_t i = (size_t)blockIdx.x * BE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 idx = key_index[i];
    u32 w[8];
    load32(w, keys, idx < K ? idx : 0);
    store32(pk, i, w);
    if (idx >= K) atomicOr(&state[0], 1u);
}

namespace {

// Measured on MI355X (tools/verify_batch_rate.py, profiles/verify_batch_rate.txt; per-element path / best equation, ms): 2^16 0.82 / 1.67, 2^17 1.45 / 1.98, 2^18 2.74 / 2.74, 2^19 5.11 / 4.16, 2^20 9.77 / 7.17
// -- the equation wins from 2^19 by more than the rounds' spread (2^18 is a tie).  Fastest width: c = 10 up to 2^15 (c = 8 ties at
// 2^10), c = 13 from 2^16.
constexpr long BATCH_EQ_MIN_DEFAULT = 1L << 19;
inline int batcheq_width(size_t n)
{
    const long v = c25519_host::tunable(c25519_host::T_BATCH_EQ_WINDOW);
    if (v >= MSM_C_MIN && v <= MSM_C_MAX) return (int)v;
    return n < ((size_t)1 << 16) ? 10 : 13;
}
inline BatchEqShape batcheq_shape(size_t n)
{
    return msm_shape(batcheq_width(n));
}
inline bool batcheq_for(size_t n)
{
    const long v = c25519_host::tunable(c25519_host::T_BATCH_EQ_MIN);
    const long mn = v == c25519_host::T_UNSET ? BATCH_EQ_MIN_DEFAULT : v;
    return mn > 0 && n >= (size_t)mn;
}
inline size_t batcheq_blocks(size_t n) { return (n + BE_BLOCK - 1) / BE_BLOCK; }

// the equation's scratch in slab order (its size is the formula of include/curve25519_amd.h); zeroed_words: flags, counts, cursor and
// reject are one run, zeroed by one fill
struct BatchEqParts { BatchEqScratch s; size_t zeroed_words; };
inline BatchEqParts batcheq_layout(Carve& c, size_t n, const BatchEqShape& sh)
{
    const size_t K = (size_t)(sh.wa + 1) * sh.buckets;
    BatchEqParts p;
    BatchEqScratch& s = p.s;
    s.rows = c.take(2 * n * MSM_ROW_WORDS);
    s.buckets = c.take(K * MSM_EXT_WORDS);
    s.windows = c.take((size_t)(sh.wa + 1) * MSM_EXT_WORDS);
    s.sc = c.take(16 * n);
    s.entries = c.take(n * (sh.wa + sh.wz));
    s.partial = c.take(16 * batcheq_blocks(n));
    const size_t run = c.words();
    s.flags = c.take4(n);
    s.counts = c.take(K);
    s.cursor = c.take(K);
    s.reject = c.take(4);                                    // one word used
    p.zeroed_words = c.words() - run;
    return p;
}

thread_local long tl_batch_last_equation = -1;

// the equation for n >= 1 elements whose first one has index index0 in the call; result: one int, or point_out: enc(T)
int batcheq_equation(int* result, void* point_out, const void* sig, const void* pk, Msgs msgs, size_t n, const BatchEqSeed& seed,
                     unsigned long long index0, hipStream_t stream)
{
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    const BatchEqShape sh = batcheq_shape(n);
    const unsigned K = (unsigned)((sh.wa + 1) * sh.buckets);
    BatchEqParts parts;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&parts, lease, stream, [&](Carve& c) { return batcheq_layout(c, n, sh); }));
    const BatchEqScratch& s = parts.s;
    C25519_TRY(hipMemsetAsync(s.flags, 0, parts.zeroed_words * sizeof(u32), stream));
    k_ed25519_batcheq_points<<<grid_for(2 * n, ED_BLOCK), ED_BLOCK, 0, stream>>>(s, sig, pk, n);
    C25519_TRY(hipGetLastError());
    const unsigned blocks = (unsigned)batcheq_blocks(n);
    k_ed25519_batcheq_scalars<<<blocks, BE_BLOCK, 0, stream>>>(s, sig, pk, msgs, n, seed, index0, sh);
    C25519_TRY(hipGetLastError());
    // points per workgroup of the digit passes: enough that a workgroup's trips to the global counters (one per bucket it touched) are
    // few beside its points
    const unsigned pts = std::max(BE_BLOCK, 2 * sh.buckets);
    const dim3 dgrid(grid_for(2 * n, (int)pts), (unsigned)sh.wa + 1);
    k_ed25519_batcheq_count<<<dgrid, BE_BLOCK, 0, stream>>>(s, n, pts, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_scan<<<1, BE_SCAN_BLOCK, 0, stream>>>(s, K);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_scatter<<<dgrid, BE_BLOCK, 0, stream>>>(s, n, pts, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_buckets<<<grid_for(K, ED_BLOCK), ED_BLOCK, 0, stream>>>(s, K);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_windows<<<(unsigned)sh.wa + 1, 64, 0, stream>>>(s, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_tail<<<1, 128, 0, stream>>>(s, sh, blocks, wide, result, point_out);
    C25519_TRY(hipGetLastError());
    return lease.release();
}

// the per-element paths' scratch: ed25519_VerifySignature_zip215_dev's own, which that call runs on, then the verdicts, the AND's two
// state words and, for the coalesced call, the n gathered keys
struct PerElementScratch { u32* inner; int* verdict; u32 *state, *pk; };
inline PerElementScratch per_element_layout(Carve& c, size_t n, bool gathered_keys)
{
    PerElementScratch p;
    p.inner = inner_verify_scratch(c, n);
    p.verdict = (int*)c.take4(n);
    p.state = c.take(4);                                     // two words used
    p.pk = c.take(gathered_keys ? 8 * n : 0);
    return p;
}

// below BATCH_EQ_MIN: ed25519_VerifySignature_zip215_dev, then the AND
int batcheq_per_element(int* result, const void* sig, const void* pk, Msgs msgs, size_t n, hipStream_t stream)
{
    PerElementScratch p;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&p, lease, stream, [n](Carve& c) { return per_element_layout(c, n, false); }));
    C25519_TRY(hipMemsetAsync(p.state, 0, 2 * sizeof(u32), stream));
    C25519_RC(verify_dev(p.verdict, sig, pk, msgs, n, stream, RULES_ZIP215, /* last_in_call = */ false, p.inner));   // the AND below is
    k_ed25519_batcheq_and<<<std::min(grid_for(n, BE_AND_BLOCK), 256u), BE_AND_BLOCK, 0, stream>>>(result, p.verdict, n, p.state);
    C25519_TRY(hipGetLastError());
    return lease.release();
}

// one equation takes at most 2^26 elements: its index entries (point * 2 + sign, n (wa + wz) of them) are addressed with 32 bits
constexpr size_t BATCH_EQ_MAX_N = (size_t)1 << 26;

// result_is_ours: `result` is this library's own pinned word (a piece of a host call), not a caller's device pointer
int batcheq_dev(void* result, const void* sig, const void* pk, Msgs msgs, size_t n, const unsigned char* seed, unsigned long long index0,
                hipStream_t stream, bool result_is_ours = false)
{
    if (!seed) return bad_arg("null seed");
    if (n > BATCH_EQ_MAX_N) return bad_arg("batch too large for one call (n > 2^26)");
    if (int rc = check_dev_args(n, { result_is_ours ? nullptr : result, sig, pk })) return rc;
    if (n == 0) {                                            // the empty AND
        k_ed25519_batcheq_and<<<1, BE_AND_BLOCK, 0, stream>>>((int*)result, nullptr, 0, nullptr);
        C25519_TRY(hipGetLastError());
        return 0;
    }
    const bool eq = batcheq_for(n);                          // (a piece of a pipelined call decides for itself: one equation per piece)
    tl_batch_last_equation = eq ? 1 : 0;
    if (!eq) return batcheq_per_element((int*)result, sig, pk, msgs, n, stream);
    BatchEqSeed sd;
    memcpy(sd.w, seed, 32);
    return batcheq_equation((int*)result, nullptr, sig, pk, msgs, n, sd, index0, stream);
}

int batcheq_fresh_seed(unsigned char (&seed)[32])
{
    size_t have = 0;
    while (have < sizeof seed) {
        const ssize_t got = getrandom(seed + have, sizeof seed - have, 0);
        if (got < 0) {
            if (errno == EINTR) continue;
            return bad_arg("getrandom(2) failed: pass a seed");
        }
        have += (size_t)got;
    }
    return 0;
}

// ---- the coalesced equation: host side ----
// Measured on MI355X (tools/verify_batch_indexed_rate.py, profiles/verify_batch_indexed_rate.txt; K <= 65536 keys; per-element call on
// the gathered keys / un-indexed equation / this one, ms): 2^17 1.45-1.48 / 1.95-2.05 / 1.94-2.00, 2^18 2.70-2.75 / 2.70-2.78 / 2.46-2.53,
// 2^19 5.12-5.17 / 4.06-4.16 / 3.38-3.51, 2^20 9.66-9.79 / 7.05-7.22 / 5.51-5.59 -- this one wins from 2^18 by more than the rounds' spread
// at every such K.  K = n (nothing merges) costs 0.25-0.27 ms over the un-indexed equation at 2^19 and 2^20 and wins from 2^19 only.  The
// faster width is the un-indexed call's in every cell (batcheq_width).
constexpr long BATCH_EQ_INDEXED_MIN_DEFAULT = 1L << 18;
inline bool keyeq_for(size_t n)
{
    const long mn = c25519_host::tunable_or(c25519_host::T_BATCH_EQ_INDEXED_MIN, BATCH_EQ_INDEXED_MIN_DEFAULT);
    return mn > 0 && n >= (size_t)mn;
}

// the coalesced equation's scratch in slab order (its size is the formula of include/curve25519_amd.h); zeroed_words: keysum, flags,
// counts, cursor and reject are one run, zeroed by one fill
struct KeyEqScratch { BatchEqScratch s; unsigned long long* keysum; size_t zeroed_words; };
inline KeyEqScratch keyeq_layout(Carve& c, size_t n, size_t K, const BatchEqShape& sh)
{
    const size_t KB = (size_t)(sh.wa + 1) * sh.buckets, N = K + n;
    KeyEqScratch k;
    BatchEqScratch& s = k.s;
    s.rows = c.take(N * MSM_ROW_WORDS);
    s.buckets = c.take(KB * MSM_EXT_WORDS);
    s.windows = c.take((size_t)(sh.wa + 1) * MSM_EXT_WORDS);
    s.sc = c.take(8 * N);
    s.partial = c.take(16 * batcheq_blocks(n));
    const size_t run = c.words();
    k.keysum = reinterpret_cast<unsigned long long*>(c.take(16 * K));   // (an even number of words from the slab's start: 64-bit sums)
    s.flags = c.take4(N);
    s.counts = c.take(KB);
    s.cursor = c.take(KB);
    s.reject = c.take(4);                                    // one word used
    k.zeroed_words = c.words() - run;
    s.entries = c.take(n * sh.wz + K * sh.wa);
    return k;
}

// the coalesced equation for n >= 1 elements over K >= 1 keys; result: one int, or point_out: enc(T)
int keyeq_equation(int* result, void* point_out, const void* keys, size_t K, const void* key_index, const void* sig, Msgs msgs, size_t n,
                   const BatchEqSeed& seed, unsigned long long index0, hipStream_t stream)
{
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    const BatchEqShape sh = batcheq_shape(n);
    const unsigned KB = (unsigned)((sh.wa + 1) * sh.buckets);
    const size_t N = K + n;
    KeyEqScratch k;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&k, lease, stream, [&](Carve& c) { return keyeq_layout(c, n, K, sh); }));
    const BatchEqScratch& s = k.s;
    C25519_TRY(hipMemsetAsync(k.keysum, 0, k.zeroed_words * sizeof(u32), stream));
    k_ed25519_keyeq_points<<<grid_for(N, ED_BLOCK), ED_BLOCK, 0, stream>>>(s, sig, keys, K, n);
    C25519_TRY(hipGetLastError());
    const unsigned blocks = (unsigned)batcheq_blocks(n);
    k_ed25519_keyeq_scalars<<<blocks, BE_BLOCK, 0, stream>>>(s, k.keysum, sig, keys, (const u32*)key_index, msgs, n, K, seed, index0, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_keyeq_fold<<<grid_for(K, BE_BLOCK), BE_BLOCK, 0, stream>>>(s, k.keysum, K, n, sh);
    C25519_TRY(hipGetLastError());
    const unsigned pts = std::max(BE_BLOCK, 2 * sh.buckets);                      // (as batcheq_equation)
    const dim3 dgrid(grid_for(N, (int)pts), (unsigned)sh.wa + 1);
    k_ed25519_keyeq_count<<<dgrid, BE_BLOCK, 0, stream>>>(s, K, n, pts, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_scan<<<1, BE_SCAN_BLOCK, 0, stream>>>(s, KB);
    C25519_TRY(hipGetLastError());
    k_ed25519_keyeq_scatter<<<dgrid, BE_BLOCK, 0, stream>>>(s, K, n, pts, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_buckets<<<grid_for(KB, ED_BLOCK), ED_BLOCK, 0, stream>>>(s, KB);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_windows<<<(unsigned)sh.wa + 1, 64, 0, stream>>>(s, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_tail<<<1, 128, 0, stream>>>(s, sh, blocks, wide, result, point_out);
    C25519_TRY(hipGetLastError());
    return lease.release();
}

// below BATCH_EQ_INDEXED_MIN: the keys gathered behind batcheq_per_element's layout, then that path
int keyeq_per_element(int* result, const void* keys, size_t K, const void* key_index, const void* sig, Msgs msgs, size_t n, hipStream_t stream)
{
    PerElementScratch p;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&p, lease, stream, [n](Carve& c) { return per_element_layout(c, n, true); }));
    C25519_TRY(hipMemsetAsync(p.state, 0, 2 * sizeof(u32), stream));
    k_ed25519_keyeq_gather<<<grid_for(n, BE_BLOCK), BE_BLOCK, 0, stream>>>(p.pk, keys, (const u32*)key_index, n, K, p.state);
    C25519_TRY(hipGetLastError());
    C25519_RC(verify_dev(p.verdict, sig, p.pk, msgs, n, stream, RULES_ZIP215, /* last_in_call = */ false, p.inner));
    k_ed25519_batcheq_and<<<std::min(grid_for(n, BE_AND_BLOCK), 256u), BE_AND_BLOCK, 0, stream>>>(result, p.verdict, n, p.state);
    C25519_TRY(hipGetLastError());
    return lease.release();
}

int keyeq_check_counts(size_t n, size_t n_key)
{
    if (n > BATCH_EQ_MAX_N) return bad_arg("batch too large for one call (n > 2^26)");
    if (n_key > BATCH_EQ_MAX_N) return bad_arg("too many keys for one call (n_key > 2^26)");
    if (n && !n_key) return bad_arg("no keys");
    return 0;
}

int keyeq_dev(void* result, const void* keys, size_t n_key, const void* key_index, const void* sig, Msgs msgs, size_t n,
              const unsigned char* seed, unsigned long long index0, hipStream_t stream, bool result_is_ours = false)
{
    if (!seed) return bad_arg("null seed");
    C25519_RC(keyeq_check_counts(n, n_key));
    if (int rc = check_dev_args(n, { result_is_ours ? nullptr : result, keys, key_index, sig })) return rc;
    if (n == 0) {                                            // the empty AND
        k_ed25519_batcheq_and<<<1, BE_AND_BLOCK, 0, stream>>>((int*)result, nullptr, 0, nullptr);
        C25519_TRY(hipGetLastError());
        return 0;
    }
    const bool eq = keyeq_for(n);
    tl_batch_last_equation = eq ? 1 : 0;
    if (!eq) return keyeq_per_element((int*)result, keys, n_key, key_index, sig, msgs, n, stream);
    BatchEqSeed sd;
    memcpy(sd.w, seed, 32);
    return keyeq_equation((int*)result, nullptr, keys, n_key, key_index, sig, msgs, n, sd, index0, stream);
}

}  // namespace

// (msm_stages.cuh) the digit passes with the key / R boundary at N (every point a key, flags[p] its own: the coalesced equation's form
// with no element), then the scan, the buckets and the windows over the wa windows in use
int c25519_engine::batcheq_bucket_stages(const BatchEqScratch& s, size_t N, const BatchEqShape& sh, hipStream_t stream)
{
    const unsigned KB = (unsigned)(sh.wa * sh.buckets);
    const unsigned pts = std::max(BE_BLOCK, 2 * sh.buckets);                      // (as batcheq_equation)
    const dim3 dgrid(grid_for(N, (int)pts), (unsigned)sh.wa);
    k_ed25519_keyeq_count<<<dgrid, BE_BLOCK, 0, stream>>>(s, N, 0, pts, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_scan<<<1, BE_SCAN_BLOCK, 0, stream>>>(s, KB);
    C25519_TRY(hipGetLastError());
    k_ed25519_keyeq_scatter<<<dgrid, BE_BLOCK, 0, stream>>>(s, N, 0, pts, sh);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_buckets<<<grid_for(KB, ED_BLOCK), ED_BLOCK, 0, stream>>>(s, KB);
    C25519_TRY(hipGetLastError());
    k_ed25519_batcheq_windows<<<(unsigned)sh.wa, 64, 0, stream>>>(s, sh);
    C25519_TRY(hipGetLastError());
    return 0;
}

extern "C" {

size_t ed25519_VerifyBatch_scratch_bytes(size_t n) { return layout_bytes([n](Carve& c) { return batcheq_layout(c, n, batcheq_shape(n)); }); }

long c25519_amd_verify_batch_last_equation(void) { return tl_batch_last_equation; }

int ed25519_VerifyBatch_zip215_dev(void* result, const void* sig, const void* pk, const void* msg, size_t msg_size, size_t n,
                                   const unsigned char* seed, void* stream)
{
    C25519_API_CALL();
    if (!result || !sig || !pk || (!msg && msg_size)) return bad_arg("null pointer");
    return batcheq_dev(result, sig, pk, fixed_msgs(msg, msg_size), n, seed, 0, (hipStream_t)stream);
}

int ed25519_VerifyBatch_zip215_ragged_dev(void* result, const void* sig, const void* pk, const void* msgs, const uint64_t* offsets,
                                          size_t n, const unsigned char* seed, void* stream)
{
    C25519_API_CALL();
    if (!result || !sig || !pk || !offsets) return bad_arg("null pointer");
    return batcheq_dev(result, sig, pk, ragged_msgs(msgs, offsets), n, seed, 0, (hipStream_t)stream);
}

// test hook: enc(T) of the point inside [8](...), always by the equation's kernels; device pointers
int c25519_amd_verify_batch_point_dev(void* out, const void* sig, const void* pk, const void* msg, size_t msg_size, size_t n,
                                      const unsigned char* seed, void* stream)
{
    C25519_API_CALL();
    if (!out || !sig || !pk || (!msg && msg_size) || !seed) return bad_arg("null pointer");
    if (n == 0) return bad_arg("the hook takes n >= 1");
    if (n > BATCH_EQ_MAX_N) return bad_arg("batch too large for one call (n > 2^26)");
    if (int rc = check_dev_args(n, { out, sig, pk })) return rc;
    BatchEqSeed sd;
    memcpy(sd.w, seed, 32);
    return batcheq_equation(nullptr, out, sig, pk, fixed_msgs(msg, msg_size), n, sd, 0, (hipStream_t)stream);
}

// The host forms.  Every piece of the pipeline writes its one int straight into a pinned word of the calling thread (kernels reach
// page-locked host memory, as the zero-copy calls of a few elements do); the pipeline returns when the last piece has completed, the
// call ANDs the words, and only then touches `verdict`: all ones, or the per-element call's verdicts.
namespace {
struct PieceResults {
    int* word = nullptr;
    size_t cap = 0;
    int reserve(size_t pieces)
    {
        if (pieces <= cap) return 0;
        if (word) C25519_TRY(hipHostFree(word));
        word = nullptr; cap = 0;
        const size_t want = pieces < 64 ? 64 : pieces;
        C25519_TRY(hipHostMalloc((void**)&word, want * sizeof(int), hipHostMallocDefault));
        cap = want;
        return 0;
    }
    ~PieceResults() { if (word && c25519_host::runtime_alive().load()) (void)hipHostFree(word); }
};
thread_local PieceResults tl_piece_results;

int batcheq_finish(int* all_valid, int* verdict, size_t pieces, size_t n)
{
    int ok = 1;
    for (size_t c = 0; c < pieces; c++) ok &= tl_piece_results.word[c] == 1;
    *all_valid = ok;
    if (verdict && ok)
        for (size_t i = 0; i < n; i++) verdict[i] = 1;
    return ok;
}
}  // namespace

int ed25519_VerifyBatch_zip215_batch(int* all_valid, int* verdict, const unsigned char* sig, const unsigned char* pk,
                                     const unsigned char* msg, size_t msg_size, size_t n, const unsigned char* seed)
{
    C25519_API_CALL();
    if (!all_valid || !sig || !pk || (!msg && msg_size)) return bad_arg("null pointer");
    *all_valid = 1;
    if (n == 0) return 0;
    unsigned char fresh[32];
    if (!seed) { C25519_RC(batcheq_fresh_seed(fresh)); seed = fresh; }
    C25519_RC(tls().ensure());
    const size_t chunk = c25519_host::piece_rows(n, 64 + 32 + msg_size);      // (run_batch's own cut of these three arrays)
    C25519_RC(tl_piece_results.reserve((n + chunk - 1) / chunk));
    size_t pieces = 0;
    C25519_RC(run_batch(n, { Arr{ sig, nullptr, 64 }, Arr{ pk, nullptr, 32 }, Arr{ msg, nullptr, msg_size } },
                        [&](void** d, size_t c, size_t lo, hipStream_t st) -> int {
                            if (pieces >= tl_piece_results.cap) return bad_arg("internal: more pieces than result words");
                            int* word = tl_piece_results.word + pieces++;
                            *word = 0;
                            return batcheq_dev(word, d[0], d[1], fixed_msgs(d[2], msg_size), c, seed, lo, st, true);
                        }));
    if (!batcheq_finish(all_valid, verdict, pieces, n) && verdict)
        return ed25519_VerifySignature_zip215_batch(verdict, sig, pk, msg, msg_size, n);
    return 0;
}

int ed25519_VerifyBatch_zip215_ragged_batch(int* all_valid, int* verdict, const unsigned char* sig, const unsigned char* pk,
                                            const unsigned char* msgs, const uint64_t* offsets, size_t n, const unsigned char* seed)
{
    C25519_API_CALL();
    if (!all_valid || !sig || !pk || !offsets) return bad_arg("null pointer");
    *all_valid = 1;
    if (n == 0) return 0;
    unsigned char fresh[32];
    if (!seed) { C25519_RC(batcheq_fresh_seed(fresh)); seed = fresh; }
    C25519_RC(tls().ensure());
    C25519_RC(tl_piece_results.reserve(1));
    tl_piece_results.word[0] = 0;
    C25519_RC(run_ragged(n, { Arr{ sig, nullptr, 64 }, Arr{ pk, nullptr, 32 } }, msgs, offsets,
                         [&](void** d, hipStream_t st) -> int {
                             return batcheq_dev(tl_piece_results.word, d[0], d[1], ragged_msgs(d[2], d[3]), n, seed, 0, st, true);
                         }));
    if (!batcheq_finish(all_valid, verdict, 1, n) && verdict)
        return ed25519_VerifySignature_zip215_ragged_batch(verdict, sig, pk, msgs, offsets, n);
    return 0;
}

// ---- the coalesced forms: keys[key_index[i]] is element i's key ----

size_t ed25519_VerifyBatch_indexed_scratch_bytes(size_t n, size_t n_key)
{
    return layout_bytes([=](Carve& c) { return keyeq_layout(c, n, n_key, batcheq_shape(n)); });
}

int ed25519_VerifyBatch_zip215_indexed_dev(void* result, const void* keys, size_t n_key, const void* key_index, const void* sig,
                                           const void* msg, size_t msg_size, size_t n, const unsigned char* seed, void* stream)
{
    C25519_API_CALL();
    if (!result || !keys || !key_index || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    return keyeq_dev(result, keys, n_key, key_index, sig, fixed_msgs(msg, msg_size), n, seed, 0, (hipStream_t)stream);
}

int ed25519_VerifyBatch_zip215_indexed_ragged_dev(void* result, const void* keys, size_t n_key, const void* key_index, const void* sig,
                                                  const void* msgs, const uint64_t* offsets, size_t n, const unsigned char* seed, void* stream)
{
    C25519_API_CALL();
    if (!result || !keys || !key_index || !sig || !offsets) return bad_arg("null pointer");
    return keyeq_dev(result, keys, n_key, key_index, sig, ragged_msgs(msgs, offsets), n, seed, 0, (hipStream_t)stream);
}

// test hook: enc(T) of the COALESCED point, always by the equation's kernels; device pointers
int c25519_amd_verify_batch_indexed_point_dev(void* out, const void* keys, size_t n_key, const void* key_index, const void* sig,
                                              const void* msg, size_t msg_size, size_t n, const unsigned char* seed, void* stream)
{
    C25519_API_CALL();
    if (!out || !keys || !key_index || !sig || (!msg && msg_size) || !seed) return bad_arg("null pointer");
    if (n == 0) return bad_arg("the hook takes n >= 1");
    C25519_RC(keyeq_check_counts(n, n_key));
    if (int rc = check_dev_args(n, { out, keys, key_index, sig })) return rc;
    BatchEqSeed sd;
    memcpy(sd.w, seed, 32);
    return keyeq_equation(nullptr, out, keys, n_key, key_index, sig, fixed_msgs(msg, msg_size), n, sd, 0, (hipStream_t)stream);
}

namespace {
// what a host form does before any work: the counts, every index, then the keys' upload into the calling thread's kept array
int keyeq_prepare(void** dkeys, const unsigned char* keys, size_t n_key, const uint32_t* key_index, size_t n)
{
    C25519_RC(keyeq_check_counts(n, n_key));
    for (size_t i = 0; i < n; i++)
        if (key_index[i] >= n_key) return bad_arg("key index out of range");
    C25519_RC(tls().ensure());
    return tls().bkeys.upload(dkeys, keys, n_key * 32);
}

// the verdicts of a failed batch: ed25519_VerifySignature_zip215_*batch on the gathered keys
std::vector<unsigned char> keyeq_gathered(const unsigned char* keys, const uint32_t* key_index, size_t n)
{
    std::vector<unsigned char> pk(n * 32);
    for (size_t i = 0; i < n; i++) memcpy(&pk[32 * i], keys + 32 * (size_t)key_index[i], 32);
    return pk;
}
}  // namespace

int ed25519_VerifyBatch_zip215_indexed_batch(int* all_valid, int* verdict, const unsigned char* keys, size_t n_key, const uint32_t* key_index,
                                             const unsigned char* sig, const unsigned char* msg, size_t msg_size, size_t n,
                                             const unsigned char* seed)
{
    C25519_API_CALL();
    if (!all_valid || !keys || !key_index || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    if (n == 0) { *all_valid = 1; return 0; }
    void* dkeys = nullptr;
    C25519_RC(keyeq_prepare(&dkeys, keys, n_key, key_index, n));
    *all_valid = 1;
    unsigned char fresh[32];
    if (!seed) { C25519_RC(batcheq_fresh_seed(fresh)); seed = fresh; }
    const size_t chunk = c25519_host::piece_rows(n, 64 + sizeof(uint32_t) + msg_size);    // (run_batch's own cut of these three arrays)
    C25519_RC(tl_piece_results.reserve((n + chunk - 1) / chunk));
    size_t pieces = 0;
    C25519_RC(run_batch(n, { Arr{ sig, nullptr, 64 }, Arr{ key_index, nullptr, sizeof(uint32_t) }, Arr{ msg, nullptr, msg_size } },
                        [&](void** d, size_t c, size_t lo, hipStream_t st) -> int {
                            if (pieces >= tl_piece_results.cap) return bad_arg("internal: more pieces than result words");
                            int* word = tl_piece_results.word + pieces++;
                            *word = 0;
                            return keyeq_dev(word, dkeys, n_key, d[1], d[0], fixed_msgs(d[2], msg_size), c, seed, lo, st, true);
                        }));
    if (!batcheq_finish(all_valid, verdict, pieces, n) && verdict)
        return ed25519_VerifySignature_zip215_batch(verdict, sig, keyeq_gathered(keys, key_index, n).data(), msg, msg_size, n);
    return 0;
}

int ed25519_VerifyBatch_zip215_indexed_ragged_batch(int* all_valid, int* verdict, const unsigned char* keys, size_t n_key,
                                                    const uint32_t* key_index, const unsigned char* sig, const unsigned char* msgs,
                                                    const uint64_t* offsets, size_t n, const unsigned char* seed)
{
    C25519_API_CALL();
    if (!all_valid || !keys || !key_index || !sig || !offsets) return bad_arg("null pointer");
    if (n == 0) { *all_valid = 1; return 0; }
    void* dkeys = nullptr;
    C25519_RC(keyeq_prepare(&dkeys, keys, n_key, key_index, n));
    *all_valid = 1;
    unsigned char fresh[32];
    if (!seed) { C25519_RC(batcheq_fresh_seed(fresh)); seed = fresh; }
    C25519_RC(tl_piece_results.reserve(1));
    tl_piece_results.word[0] = 0;
    C25519_RC(run_ragged(n, { Arr{ sig, nullptr, 64 }, Arr{ key_index, nullptr, sizeof(uint32_t) } }, msgs, offsets,
                         [&](void** d, hipStream_t st) -> int {
                             return keyeq_dev(tl_piece_results.word, dkeys, n_key, d[1], d[0], ragged_msgs(d[2], d[3]), n, seed, 0, st, true);
                         }));
    if (!batcheq_finish(all_valid, verdict, 1, n) && verdict)
        return ed25519_VerifySignature_zip215_ragged_batch(verdict, sig, keyeq_gathered(keys, key_index, n).data(), msgs, offsets, n);
    return 0;
}

}  // extern "C"
