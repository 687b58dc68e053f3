// curve25519_amd/csrc/engine_msm.hip -- ed25519_MultiScalarMult[_vartime]_*, ristretto255_MultiScalarMult[_vartime]_*: n_groups
// independent sums of m terms each, Q_g = sum_i [s_i mod L] P_i (the lane's work: msm_sum.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "msm_sum.cuh"
#include "msm_stages.cuh"

// The constant-time path is three stages over one lease: k_msm_rows (one lane per row: the group calls' walk at two waves per SIMD),
// k_msm_sum as often as it takes to bring every group down to one point (each pass divides a group by MSM_SUM_CHUNK), k_msm_finish
// (one lane per group; the Edwards encoding then goes through the shared inversion, the ristretto255 one is the lane's own chain).
// The bucket path runs per group, one after the other over the same scratch: k_msm_clear, k_msm_points and k_msm_scalars, the batch equation's
// count / scan / scatter / buckets / windows kernels as they are (msm_stages.cuh), k_msm_tail.
constexpr int MSM_BLOCK = 256;

template <int G>
__global__ void __launch_bounds__(MSM_BLOCK, 2) k_msm_rows(u32* pts, u32* flags, const void* scalar, const void* point, size_t n)
{
    const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 sw[8], pw[8];
    load32(sw, scalar, i);
    load32(pw, point, i);
    ge_ext S;
    const u32 ok = msm_sum_row_lane<G, MSM_WALK_WINDOW>(S, sw, pw);
    msm_store_ext(pts + i * MSM_EXT_WORDS, S);
    flags[i] = ok;
}

// one pass: every group's m_in points -> per = ceil(m_in / MSM_SUM_CHUNK) points; lane t of the n_groups * per owns chunk t mod per of
// group t / per
__global__ void __launch_bounds__(MSM_BLOCK, 2) k_msm_sum(u32* dst, u32* dflags, const u32* __restrict__ src, const u32* __restrict__ sflags,
                                                         size_t m_in, size_t per, size_t total)
{
    const size_t t = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
    if (t >= total) return;
    const size_t g = t / per, j = t - g * per, at = j * MSM_SUM_CHUNK;
    const u32 count = (u32)(m_in - at < (size_t)MSM_SUM_CHUNK ? m_in - at : (size_t)MSM_SUM_CHUNK);
    ge_ext S;
    const u32 ok = msm_sum_chunk_lane(S, src, sflags, g * m_in + at, count);
    msm_store_ext(dst + t * MSM_EXT_WORDS, S);
    dflags[t] = ok;
}

// one lane per group.  Edwards: X, Y, Z and the ok word to the scratch, k_batch_invert<FinishGroupPoint> writes q.  ristretto255: q.
template <int G>
__global__ void __launch_bounds__(MSM_BLOCK, 2) k_msm_finish(ProjScratch scr, u32* okw, void* q, int* ok, const u32* __restrict__ pts,
                                                            const u32* __restrict__ flags, size_t n)
{
    const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
    if (i >= n) return;
    ge_ext S;
    msm_load_ext(S, pts + i * MSM_EXT_WORDS);
    const u32 keep = flags[i];
    ok[i] = (int)(keep & 1u);
    if constexpr (G == MSM_GROUP_EDWARDS) {
        store_proj(scr, n, i, S);
        okw[i] = keep;
    } else {
        u32 out[8];
        rist_encode<true>(out, S);
#pragma unroll
        for (int j = 0; j < 8; j++) out[j] &= keep;
        store32(q, i, out);
    }
}

// ---- the bucket path: rows first .. first + N - 1 of the call are one group ----

// flags, counts, cursor and the reject word before every group.  A kernel of the call's own, not a fill: a captured call is then a
// chain of kernel nodes alone, like every call the graph tests replay (a captured call whose groups were separated by fills faulted
// when it was replayed, where the same call run directly gave the model's bytes).
__global__ void __launch_bounds__(MSM_BLOCK) k_msm_clear(u32* p, size_t words)
{
    const size_t i = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
    if (i < words) p[i] = 0;
}

__global__ void __launch_bounds__(MSM_BLOCK) k_msm_scalars(BatchEqScratch s, const void* scalar, size_t first, size_t N, int c)
{
    const size_t j = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
    if (j >= N) return;
    u32 sw[8], k[8];
    load32(sw, scalar, first + j);
    msm_sum_biased_scalar(k, sw, c);
    soa_store8(s.sc, N, j, k);
}

template <int G>
__global__ void __launch_bounds__(MSM_BLOCK, 2) k_msm_points(BatchEqScratch s, const void* point, size_t first, size_t N)
{
    const size_t j = (size_t)blockIdx.x * MSM_BLOCK + threadIdx.x;
    if (j >= N) return;
    u32 w[8], row[24];
    load32(w, point, first + j);
    const u32 ok = msm_sum_point_row<G>(row, w);
    uint4* out = reinterpret_cast<uint4*>(s.rows + j * MSM_ROW_WORDS);
#pragma unroll
    for (int g = 0; g < 6; g++) out[g] = make_uint4(row[4 * g], row[4 * g + 1], row[4 * g + 2], row[4 * g + 3]);
    if (!ok) { s.flags[j] = 1u; atomicOr(s.reject, 1u); }
}

// one lane: Horner over the windows, the group's encoding, the verdict of group `g`
template <int G>
__global__ void __launch_bounds__(64) k_msm_tail(BatchEqScratch s, BatchEqShape shape, void* q, int* ok, size_t g)
{
    if (threadIdx.x != 0) return;
    ge_ext T;
    msm_sum_horner(T, s.windows, shape);
    u32 out[8];
    msm_sum_encode<G>(out, T);
    const u32 keep = *s.reject ? 0u : 0xffffffffu;
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] &= keep;
    store32(q, g, out);
    ok[g] = (int)(keep & 1u);
}

namespace {

// one group takes at most 2^26 rows (the bucket path's index entries, point * 2 + sign, m * wa of them, are addressed with 32 bits),
// one call at most 2^31 (check_dev_args)
constexpr size_t MSM_MAX_M = (size_t)1 << 26;
constexpr size_t MSM_MAX_ROWS = (size_t)1 << 31;

// Measured on MI355X (tools/msm_rate.py, profiles/msm_rate.txt; one group, plain call / bucket path at its best width, ms; Edwards, the
// ristretto255 figures are within 8 %): 2^10 1.13 / 0.77, 2^12 1.26 / 0.83, 2^14 1.30 / 0.97, 2^16 1.48 / 1.16, 2^18 4.13 / 1.83,
// 2^20 13.51 / 4.18 -- ONE group wins on the bucket path from the smallest measured size, 2^10, and at every larger one, by more than
// the rounds' spread.  The groups of a call run one after the other there, nine launches each, while the plain call walks all rows at
// once: 4 groups of 2^18 still win (7.2 against 13.7 ms), 16 groups of 2^16 lose (19.6 against 13.9 ms) and 256 groups of 2^12 take
// 227 ms against 13.9.  So the built-in threshold is 2^10 for one group and 2^18 for more; the tunable, where set, holds for any
// number of groups.  Fastest width: c = 10 below 2^14 (c = 9 ties at 2^10 and 2^11), c = 11 up to 2^16 (where c = 12 ties), c = 12
// from 2^17.
constexpr long MSM_BUCKET_MIN_ONE_GROUP = 1L << 10, MSM_BUCKET_MIN_MANY_GROUPS = 1L << 18;
inline int msm_width(size_t m)
{
    const long v = c25519_host::tunable(c25519_host::T_MSM_WINDOW);
    if (v >= MSM_C_MIN && v <= MSM_C_MAX) return (int)v;
    return m < ((size_t)1 << 14) ? 10 : m < ((size_t)1 << 17) ? 11 : 12;
}
inline bool msm_bucket_for(size_t m, size_t n_groups, bool vartime)
{
    const long mn = c25519_host::tunable_or(c25519_host::T_MSM_BUCKET_MIN, n_groups <= 1 ? MSM_BUCKET_MIN_ONE_GROUP : MSM_BUCKET_MIN_MANY_GROUPS);
    return vartime && mn > 0 && m >= (size_t)mn;
}
inline size_t msm_chunks(size_t m) { return (m + MSM_SUM_CHUNK - 1) / MSM_SUM_CHUNK; }

// the constant-time path's scratch: the rows' points and flags (a), what a pass leaves (b; the passes go a -> b -> a ...), and the
// Edwards finish's projective part and ok words
struct MsmSumScratch { u32 *a, *b, *fa, *fb; ProjScratch scr; u32* okw; };
inline MsmSumScratch msm_sum_layout(Carve& c, size_t m, size_t n_groups)
{
    const size_t rows = m * n_groups, after = m > 1 ? msm_chunks(m) * n_groups : 0;
    MsmSumScratch s;
    s.a = c.take(rows * MSM_EXT_WORDS);
    s.b = c.take(after * MSM_EXT_WORDS);
    s.fa = c.take4(rows);
    s.fb = c.take4(after);
    s.scr = c.proj(n_groups);
    s.okw = c.take4(n_groups);
    return s;
}

// the bucket path's scratch for ONE group of m points, K = wa * buckets counters; zeroed_words: flags, counts, cursor and reject are
// one run, cleared by k_msm_clear before every group
struct MsmBucketParts { BatchEqScratch s; size_t zeroed_words; };
inline MsmBucketParts msm_bucket_layout(Carve& c, size_t m, const BatchEqShape& sh)
{
    const size_t K = (size_t)sh.wa * sh.buckets;
    MsmBucketParts p;
    BatchEqScratch& s = p.s;
    s.rows = c.take(m * MSM_ROW_WORDS);
    s.buckets = c.take(K * MSM_EXT_WORDS);
    s.windows = c.take((size_t)sh.wa * MSM_EXT_WORDS);
    s.sc = c.take(8 * m);
    s.entries = c.take4(m * sh.wa);
    s.partial = nullptr;
    const size_t run = c.words();
    s.flags = c.take4(m);
    s.counts = c.take(K);
    s.cursor = c.take(K);
    s.reject = c.take(4);                                    // one word used
    p.zeroed_words = c.words() - run;
    return p;
}

template <int G>
int msm_sum_path(void* q, int* ok, const void* scalar, const void* point, size_t m, size_t n_groups, hipStream_t stream)
{
    MsmSumScratch s;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&s, lease, stream, [=](Carve& c) { return msm_sum_layout(c, m, n_groups); }));
    const size_t rows = m * n_groups;
    k_msm_rows<G><<<grid_for(rows, MSM_BLOCK), MSM_BLOCK, 0, stream>>>(s.a, s.fa, scalar, point, rows);
    C25519_TRY(hipGetLastError());
    u32 *src = s.a, *sflags = s.fa, *dst = s.b, *dflags = s.fb;
    for (size_t m_in = m; m_in > 1;) {
        const size_t per = msm_chunks(m_in), total = per * n_groups;
        k_msm_sum<<<grid_for(total, MSM_BLOCK), MSM_BLOCK, 0, stream>>>(dst, dflags, src, sflags, m_in, per, total);
        C25519_TRY(hipGetLastError());
        std::swap(src, dst);
        std::swap(sflags, dflags);
        m_in = per;
    }
    k_msm_finish<G><<<grid_for(n_groups, MSM_BLOCK), MSM_BLOCK, 0, stream>>>(s.scr, s.okw, q, ok, src, sflags, n_groups);
    C25519_TRY(hipGetLastError());
    if (G == MSM_GROUP_EDWARDS) C25519_RC(launch_invert(s.scr, n_groups, FinishGroupPoint{ s.scr.a, s.scr.b, s.okw, q, n_groups }, stream));
    return lease.release();
}

template <int G>
int msm_bucket_path(void* q, int* ok, const void* scalar, const void* point, size_t m, size_t n_groups, hipStream_t stream)
{
    const BatchEqShape sh = msm_shape(msm_width(m));
    MsmBucketParts parts;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&parts, lease, stream, [&](Carve& c) { return msm_bucket_layout(c, m, sh); }));
    const BatchEqScratch& s = parts.s;
    for (size_t g = 0; g < n_groups; g++) {
        k_msm_clear<<<grid_for(parts.zeroed_words, MSM_BLOCK), MSM_BLOCK, 0, stream>>>(s.flags, parts.zeroed_words);
        C25519_TRY(hipGetLastError());
        k_msm_points<G><<<grid_for(m, MSM_BLOCK), MSM_BLOCK, 0, stream>>>(s, point, g * m, m);
        C25519_TRY(hipGetLastError());
        k_msm_scalars<<<grid_for(m, MSM_BLOCK), MSM_BLOCK, 0, stream>>>(s, scalar, g * m, m, sh.c);
        C25519_TRY(hipGetLastError());
        C25519_RC(batcheq_bucket_stages(s, m, sh, stream));
        k_msm_tail<G><<<1, 64, 0, stream>>>(s, sh, q, ok, g);
        C25519_TRY(hipGetLastError());
    }
    return lease.release();
}

int msm_check_sizes(size_t m, size_t n_groups)
{
    if (m == 0) return bad_arg("m must be at least 1");
    if (m > MSM_MAX_M) return bad_arg("group too large for one call (m > 2^26)");
    if (n_groups > MSM_MAX_ROWS / m) return bad_arg("batch too large (n_groups * m > 2^31)");
    return 0;
}

template <int G>
int msm_dev(void* q, void* ok, const void* scalar, const void* point, size_t m, size_t n_groups, void* stream, bool vartime)
{
    C25519_API_CALL();
    if (!q || !ok || !scalar || !point) return bad_arg("null pointer");
    C25519_RC(msm_check_sizes(m, n_groups));
    if (int rc = check_dev_args(m * n_groups, { q, ok, scalar, point })) return rc;
    if (n_groups == 0) return 0;
    if (msm_bucket_for(m, n_groups, vartime)) return msm_bucket_path<G>(q, (int*)ok, scalar, point, m, n_groups, (hipStream_t)stream);
    return msm_sum_path<G>(q, (int*)ok, scalar, point, m, n_groups, (hipStream_t)stream);
}

}  // namespace

extern "C" {

// (the rules: include/curve25519_amd.h)  c25519_amd_last_shape is not written.

size_t c25519_MultiScalarMult_scratch_bytes(size_t m, size_t n_groups, int vartime)
{
    if (m == 0 || n_groups == 0 || m > MSM_MAX_M || n_groups > MSM_MAX_ROWS / m) return 0;
    if (msm_bucket_for(m, n_groups, vartime != 0)) return layout_bytes([=](Carve& c) { return msm_bucket_layout(c, m, msm_shape(msm_width(m))); });
    return layout_bytes([=](Carve& c) { return msm_sum_layout(c, m, n_groups); });
}

int ed25519_MultiScalarMult_dev(void* q, void* ok, const void* scalar, const void* point, size_t m, size_t n_groups, void* stream)
{
    return msm_dev<MSM_GROUP_EDWARDS>(q, ok, scalar, point, m, n_groups, stream, false);
}

int ed25519_MultiScalarMult_vartime_dev(void* q, void* ok, const void* scalar, const void* point, size_t m, size_t n_groups, void* stream)
{
    return msm_dev<MSM_GROUP_EDWARDS>(q, ok, scalar, point, m, n_groups, stream, true);
}

int ristretto255_MultiScalarMult_dev(void* q, void* ok, const void* scalar, const void* point, size_t m, size_t n_groups, void* stream)
{
    return msm_dev<MSM_GROUP_R255>(q, ok, scalar, point, m, n_groups, stream, false);
}

int ristretto255_MultiScalarMult_vartime_dev(void* q, void* ok, const void* scalar, const void* point, size_t m, size_t n_groups, void* stream)
{
    return msm_dev<MSM_GROUP_R255>(q, ok, scalar, point, m, n_groups, stream, true);
}

}  // extern "C"
