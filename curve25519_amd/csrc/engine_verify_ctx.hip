// curve25519_amd/csrc/engine_verify_ctx.hip -- Ed25519 verification against Verify_Init contexts: ed25519_Verify_Init, and every
// ed25519_Verify_Check form -- one key (shared table, two wide combs, the remembered comb), many contexts in one call (indexed), a pair
// per wave for small calls, the strict mask, the ZIP-215 coset finish -- kernels and *_dev entry points.
// It reaches the per-element unit (engine_verify.hip) through verify_dev and ed25519_VerifySignature_scratch_bytes only.
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "verify_check.cuh"
#include "verify_ctx.cuh"
#include "verify_ctx_zip215.cuh"

// ed25519_Verify_Check (k_ed25519_verify_check, verify_check.cuh) with ONE key for the whole batch (the reference's two-phase
// use: Verify_Init once, many Verify_Check calls, ed25519_verify.c:282-286).  ctx is the 2080-byte context (pk || 16 canonical
// rows); the workgroup converts it once into limb form in LDS (limb-major, 16 rows wide: the 16 possible row indices
// of a lookup fall into 16 different banks).
struct QTableLds {
    const u32* base;                                       // [40][16]
    C25519_DEV void load(ge_pe& q, u32 e) const
    {
#pragma unroll
        for (int i = 0; i < 10; i++) {
            q.ypx.v[i] = base[(i) * 16 + e];
            q.ymx.v[i] = base[(10 + i) * 16 + e];
            q.t2d.v[i] = base[(20 + i) * 16 + e];
            q.z2.v[i] = base[(30 + i) * 16 + e];
        }
    }
};

__global__ void __launch_bounds__(ED_BLOCK, 2) k_ed25519_verify_check_shared(ProjScratch scr, const void* sig,
                                                                              const u32* __restrict__ ctx, Msgs msgs,
                                                                              size_t n, const u32* __restrict__ g_tbl,
                                                                              const u32* __restrict__ wide_ok)
{
    if (wide_ok && *wide_ok) return;                       // k_ed25519_verify_check_wide decides this batch
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[PA_WORDS * 256];
    __shared__ u32 lds_q[PE_WORDS * 16];
    if (threadIdx.x < 64) {                                // 16 rows x 4 field elements
        const u32 row = threadIdx.x >> 2, f = threadIdx.x & 3;
        u32 w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = ctx[8 + row * 32 + f * 8 + j];
        fe v;
        fe_from_words(v, w);
#pragma unroll
        for (int l = 0; l < 10; l++) lds_q[(10 * f + l) * 16 + row] = v.v[l];
    }
    lds_stage_words(lds_tbl, g_tbl + REF_TBL_OFFSET, REF_TBL_WORDS);   // ends with __syncthreads()
    const size_t i = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pkw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pkw[j] = ctx[j];
    const QTableLds tbl{ lds_q };
    verify_check_lane(scr, n, i, sig, pkw, msgs, tbl, lds_tbl);
}

// ed25519_Verify_Init for a call of a few keys: one key per wave.  The square root by every lane on the same value (one lane's
// code: a cooperative one would be no faster), the table by the whole wave (coop::qtable_build_coop).  501 us per call in the
// per-lane kernel (a lone lane's 192 doublings), ~130 here.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_ed25519_verify_init_coop(const void* pk, size_t n, u32* ctx_rows /* n contexts, stride_words apart, the 16 rows of each */, size_t stride_words,
                           DoneWord done)
{
    __shared__ __attribute__((aligned(16))) u32 lds[coop::Q_LDS_WORDS];
    if (blockIdx.x >= n) return;
    u32* rows = ctx_rows + blockIdx.x * stride_words;
    coop::verify_init_one(lds, coop::make_lane(threadIdx.x), pk, blockIdx.x, rows);
    if (threadIdx.x < 8) rows[(int)threadIdx.x - 8] = ((const u32*)pk)[blockIdx.x * 8 + threadIdx.x];   // the context's first 32 bytes: the key
    if (threadIdx.x == 0) signal_done(done);               // (rows and key are this one wave's stores: the fence waits for them all)
}

// ed25519_Verify_Check for a call of a few pairs (the reference's prototype is a call of ONE): one pair per wave, the
// reference's own operation order (coop::poly_mult), one shared-nothing inversion per pair.  454 us per call in the per-lane
// kernel above (a lone lane walks 63 doublings and 96 additions); ~125 here.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_ed25519_verify_check_coop(int* verdict, const void* sig, const u32* __restrict__ ctx, Msgs msgs, size_t n, const u32* __restrict__ g_tbl,
                            DoneWord done)
{
    __shared__ __attribute__((aligned(16))) u32 lds[coop::Q_LDS_WORDS];
    if (blockIdx.x >= n) return;
    coop::verify_check_one(lds, coop::make_lane(threadIdx.x), verdict, sig, ctx, msgs, blockIdx.x, g_tbl + REF_TBL_OFFSET);
    if (threadIdx.x == 0) signal_done(done);
}

// ---- one key, a big batch: both scalars over wide combs ------------------------------------------------------------------
// With ONE key for the whole batch the double-scalar product T = s*B + h*(-A) is two FIXED-base products: the base point's
// wide comb (ge25519.cuh) and one built for -A the same way, walked together -- 39 additions and 4 doublings per signature
// instead of the reference order's 255 doublings and 95 additions (ed25519_verify.c:243-280).  For a key ON the curve any
// evaluation of the group law gives the same point T, hence the same enc(T) and the same verdict; so this path decides
// a batch only when (a) the context is byte for byte what Verify_Init computes for its key bytes (a context is caller
// storage: one that was written by anything else keeps the kernel above, which reads its rows as they are, like the
// reference) and (b) the key decompresses onto the curve.  k_ed25519_verify_ctx_prepare establishes both in block 0 -- one
// lane rebuilds the 16 rows, as Verify_Init did -- while the other blocks generate the key's comb rows (the work of
// k_gen_wide_table, 0.6 ms); worth it from 2^16 signatures per call (tunable ONE_KEY_WIDE).
// `remembered` (KEEP_CTX_WORDS + 1 words behind the key's comb, in a buffer that outlives the call): the context the comb was
// built for and a state word -- 0 nothing yet, 1 remembered but not eligible, 2 remembered and eligible.  The reference's use is
// ONE Verify_Init and MANY Verify_Check calls (ed25519_verify.c:282-286): a call whose context equals the remembered bytes skips
// all of the preparation (every block finds that out for itself: 2080 bytes out of L2); k_ed25519_verify_ctx_remember, behind
// this kernel on the stream, writes the bytes down.
constexpr int KEEP_CTX_WORDS = 2080 / 4;
// build_if_new = 0 (one block): only ask whether the context is the remembered one -- what calls below the ONE_KEY_WIDE size do:
// a remembered comb costs them nothing, a new one would cost more than they take.
__global__ void __launch_bounds__(128) k_ed25519_verify_ctx_prepare(u32* wide_key /*[WB_NT][WB_ROWS][WB_ROW_WORDS]*/, u32* check_rows /*[16][32]*/,
                                                                     u32* wide_ok, const u32* __restrict__ ctx,
                                                                     const u32* __restrict__ remembered, int build_if_new)
{
    {
        int same = remembered[KEEP_CTX_WORDS] != 0;
        for (int w = threadIdx.x; w < KEEP_CTX_WORDS; w += 128) same = same && remembered[w] == ctx[w];
        if (__syncthreads_and(same)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) *wide_ok = remembered[KEEP_CTX_WORDS] == 2 ? 1u : 0u;
            return;
        }
        if (!build_if_new) {
            if (blockIdx.x == 0 && threadIdx.x == 0) *wide_ok = 0u;
            return;
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x != 0) return;
        u32 pkw[8];
#pragma unroll
        for (int j = 0; j < 8; j++) pkw[j] = ctx[j];
        ge_ext Q;
        u32 yw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) yw[i] = pkw[i];
        const u32 parity = yw[7] >> 31;
        yw[7] &= 0x7fffffffu;
        fe_from_words(Q.Y, yw);
        const u32 on_curve = ge_calc_x_checked(Q.X, Q.Y, ~parity);     // ed_decode_neg_key, keeping the square root's verdict
        fe_mul(Q.T, Q.X, Q.Y);
        fe_set_u32(Q.Z, 1);
        qtable_build(QTableCanon{ check_rows }, Q);
        u32 diff = 0;
        for (int w = 0; w < 16 * 32; w++) diff |= check_rows[w] ^ ctx[8 + w];
        *wide_ok = (on_curve && diff == 0) ? 1u : 0u;
        return;
    }
    const u32 g = (blockIdx.x - 1) * 128 + threadIdx.x;       // table * WB_ROWS + row
    const int table = (int)(g / WB_ROWS);
    // -A in affine precomputed form = row 1 of the context (Verify_Init stores the decompressed key with Z = 1); if the context
    // is not Verify_Init's, block 0 says so and nobody reads these rows
    ge_pa P;
    {
        u32 w[8];
#pragma unroll
        for (int f = 0; f < 3; f++) {
#pragma unroll
            for (int j = 0; j < 8; j++) w[j] = ctx[8 + 32 + 8 * f + j];
            fe_from_words(f == 0 ? P.ypx : f == 1 ? P.ymx : P.t2d, w);
        }
    }
    u32 rows[3][8];
    ge_signed_comb_row_of(rows, P, g % WB_ROWS, (WB_NT - 1 - table) * WB_STEP, WB_TEETH, WB_COLS);
    uint4* out = reinterpret_cast<uint4*>(wide_key + (size_t)g * WB_ROW_WORDS);
#pragma unroll
    for (int f = 0; f < 3; f++) {
        out[2 * f] = make_uint4(rows[f][0], rows[f][1], rows[f][2], rows[f][3]);
        out[2 * f + 1] = make_uint4(rows[f][4], rows[f][5], rows[f][6], rows[f][7]);
    }
    out[6] = make_uint4(2, 0, 0, 0);                          // 2Z, as in k_gen_wide_table
    out[7] = make_uint4(0, 0, 0, 0);
}

__global__ void __launch_bounds__(128) k_ed25519_verify_ctx_remember(u32* remembered, const u32* __restrict__ ctx, const u32* __restrict__ wide_ok)
{
    for (int w = threadIdx.x; w < KEEP_CTX_WORDS; w += 128) remembered[w] = ctx[w];
    if (threadIdx.x == 0) remembered[KEEP_CTX_WORDS] = 1u + (*wide_ok ? 1u : 0u);
}

__global__ void __launch_bounds__(WB_BLOCK, 4) k_ed25519_verify_check_wide(ProjScratch scr, const void* sig, const u32* __restrict__ ctx,
                                                                          Msgs msgs, size_t n, const u32* __restrict__ wide_base,
                                                                          const u32* __restrict__ wide_key, const u32* __restrict__ wide_ok)
{
    if (!*wide_ok) return;                                 // k_ed25519_verify_check_shared decides this batch
    __shared__ unsigned short cols[2 * WB_COLS * WB_BLOCK];
    const size_t i = (size_t)blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pkw[8], Sw[8], h[8], Rw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pkw[j] = ctx[j];
    load32(Rw, sig, 2 * i);
    ed_hram(h, Rw, pkw, msgs.ptr(i), msgs.len(i));
    sc_mod(h);
    load32(Sw, sig, 2 * i + 1);                            // raw 256 bits: no s < L check (ed25519_verify.c:308)
    unsigned short* cs = cols + threadIdx.x;
    unsigned short* ch = cols + WB_COLS * WB_BLOCK + threadIdx.x;
    wb_columns(cs, WB_BLOCK, Sw);                          // s + L when even: L * B = O
    const u32 h_even = wb_columns<false>(ch, WB_BLOCK, h);    // h + 1 when even: -A may carry torsion, one -A comes off again
    ge_ext T;                                              // (-A = row 1 of the context, affine: Verify_Init's Z is 1)
    ge_double_base_mult_wide(T, wide_base, cs, wide_key, ch, WB_BLOCK, h_even, ctx + 8 + 32);
    store_proj(scr, n, i, T);
}

// ... and on FOUR lanes per pair (quad::verify_check_wide_element: an addition in two product levels, inversion, encoding and the
// comparison in the same launch) for calls of 2^10 .. 2^14 pairs -- where the one-lane kernel above leaves three quarters of the
// SIMDs idle and every lane walks the whole 0.16 ms chain: what a caller with ONE remembered key and a few thousand signatures
// per call runs (ed25519_verify.c:282-286).  16 pairs per one-wave workgroup; LDS: the lanes' parked columns of s and h.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_ed25519_verify_check_wide_quad(int* verdict, const void* sig, const u32* __restrict__ ctx, Msgs msgs, size_t n,
                                 const u32* __restrict__ wide_base, const u32* __restrict__ wide_key, const u32* __restrict__ wide_ok)
{
    if (!*wide_ok) return;                                 // k_ed25519_verify_check_shared decides this batch
    __shared__ unsigned short cols[2 * WB_COLS * 64];
    const size_t e = (size_t)blockIdx.x * quad::ELEMS_PER_WAVE + (threadIdx.x >> 2);
    if (e >= n) return;                                    // (whole quads leave)
    quad::verify_check_wide_element(verdict, sig, ctx, msgs.ptr(e), msgs.len(e), e, wide_base, wide_key, cols + threadIdx.x,
                                    cols + WB_COLS * 64 + threadIdx.x, 64);
}

// ---- many contexts in one call: element i against context ctx_index[i] (verify_ctx.cuh) ------------------------------------------
// Per lane, as k_ed25519_verify_check_shared with the element's own context: the 8-fold base table staged in LDS, the 16 rows of the
// context read from global memory at each lookup (QTableCanon: one 128-byte row, 2080k + 32 + 128r bytes into the call's contexts,
// so three of every four contexts' rows straddle two lines; C25519_INDEXED_REPACK = 1 reads an aligned copy of them instead).
__global__ void __launch_bounds__(ED_BLOCK, 2) k_ed25519_verify_check_indexed(ProjScratch scr, const void* sig, const u32* __restrict__ ctxs,
                                                                               size_t n_ctx, const u32* __restrict__ ctx_index, Msgs msgs,
                                                                               size_t n, const u32* __restrict__ g_tbl, const u32* __restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[PA_WORDS * 256];
    lds_stage_words(lds_tbl, g_tbl + REF_TBL_OFFSET, REF_TBL_WORDS);
    const size_t i = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32* ctx = indexed_ctx(ctxs, n_ctx, ctx_index, i);
#if C25519_INDEXED_REPACK
    const QTableCanon tbl{ const_cast<u32*>(rows) + (ctx ? (size_t)ctx_index[i] * QTABLE_CANON_WORDS : 0) };
#else
    (void)rows;
    const QTableCanon tbl{ const_cast<u32*>(ctx) + 8 };
#endif
    ge_ext T;
    verify_ctx_point(T, ctx, tbl, sig, msgs, i, lds_tbl);
    store_proj(scr, n, i, T);
}

#if C25519_INDEXED_REPACK
// the rows of the call's contexts, 2048 bytes per context, into `rows` (128-byte aligned): one 16-byte word per thread
__global__ void __launch_bounds__(256) k_ed25519_verify_ctx_repack(uint4* rows, const u32* __restrict__ ctxs, size_t n_ctx)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_ctx * (QTABLE_CANON_WORDS / 4)) return;
    const size_t k = g / (QTABLE_CANON_WORDS / 4), q = g % (QTABLE_CANON_WORDS / 4);
    rows[g] = reinterpret_cast<const uint4*>(ctxs + k * VCTX_WORDS + 8)[q];
}
#endif

// ... and for a call of a few pairs, one pair per wave (k_ed25519_verify_check_coop with the element's context)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_ed25519_verify_check_indexed_coop(int* verdict, const void* sig, const u32* __restrict__ ctxs, size_t n_ctx,
                                    const u32* __restrict__ ctx_index, Msgs msgs, size_t n, const u32* __restrict__ g_tbl, DoneWord done)
{
    __shared__ __attribute__((aligned(16))) u32 lds[coop::Q_LDS_WORDS];
    if (blockIdx.x >= n) return;
    const u32* ctx = indexed_ctx(ctxs, n_ctx, ctx_index, blockIdx.x);
    if (ctx)
        coop::verify_check_one(lds, coop::make_lane(threadIdx.x), verdict, sig, ctx, msgs, blockIdx.x, g_tbl + REF_TBL_OFFSET);
    else if (threadIdx.x == 0)
        verdict[blockIdx.x] = 0;
    if (threadIdx.x == 0) signal_done(done);
}

// ---- ed25519_Verify_Check_strict_*: one kernel behind the plain call's ---------------------------------------------------------
// The plain kernels decide rule 6; this one applies the others to their verdicts.  Every workgroup decides rules 2-4 for the context's
// key bytes itself -- its first wave takes the square root cooperatively (coop::strict_key_ok) -- so no word is handed from kernel to
// kernel; the grid stops at SM_MAX_BLOCKS workgroups (one square root per SIMD at most) and strides over the pairs, applying rules 1
// and 5 per pair.  Element 0's lane signals a call of one.
constexpr int SM_BLOCK = 256, SM_MAX_BLOCKS = 1024;
__global__ void __launch_bounds__(SM_BLOCK) k_ed25519_verify_check_strict_mask(int* verdict, const void* sig, size_t n,
                                                                               const u32* __restrict__ ctx, DoneWord done)
{
    __shared__ __attribute__((aligned(16))) u32 lds[coop::LDS_WORDS];
    __shared__ u32 key_ok;
    if (threadIdx.x < 64) {
        u32 w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = ctx[j];
        const u32 ok = coop::strict_key_ok(lds, coop::make_lane(threadIdx.x), w);
        if (threadIdx.x == 0) key_ok = ok;
    }
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * SM_BLOCK) {
        u32 Rw[8], Sw[8];
        load32(Rw, sig, 2 * i);
        load32(Sw, sig, 2 * i + 1);
        if (!key_ok || strict_reject_pair(Rw, Sw)) verdict[i] = 0;
        if (i == 0) signal_done(done);                     // (done: a call of ONE pair, this lane's own store in front of it)
    }
}

// ---- ed25519_Verify_Check_zip215_*: the ZIP-215 verdict against Verify_Init contexts (verify_ctx_zip215.cuh) ------------------------------
// Behind the plain calls' own walk kernels, which are launched as the plain calls launch them (no twin of a walk: a twin in this unit
// has changed their gfx950 code before).  k_ed25519_verify_coset_prep, one launch of two roles: the first `elem_blocks`
// workgroups take an element per lane and turn the T the walk left into W = Z (Z^2 + kXY)(Z^2 - kXY), in the scratch part the shared
// inversion is then pointed at (ProjScratch::prefix); the others take a CONTEXT per lane and decide rule 2 for it, one word each.
// k_batch_invert<FinishVerifyZip215> then compares the coset T + E[8] with R's bytes and writes the verdicts.
constexpr int ZC_BLOCK = 256;
__global__ void __launch_bounds__(ZC_BLOCK) k_ed25519_verify_coset_prep(ProjScratch scr, size_t n, unsigned elem_blocks,
                                                                               const u32* __restrict__ ctxs, size_t n_ctx, u32* key_ok)
{
    if (blockIdx.x < elem_blocks) {
        const size_t i = (size_t)blockIdx.x * ZC_BLOCK + threadIdx.x;
        if (i < n) coset_prep_element(scr.prefix, scr.a, scr.b, scr.z, n, i);
        return;
    }
    const size_t c = (size_t)(blockIdx.x - elem_blocks) * ZC_BLOCK + threadIdx.x;
    if (c < n_ctx) key_ok[c] = zip215_ctx_key_ok(ctxs + c * VCTX_WORDS);
}

// calls below ZIP215_CHECK_MIN: pk[i] = bytes 0..31 of element i's context (ctx_index null: of the one context) for
// ed25519_VerifySignature_zip215_dev's kernels -- the same verdict for a context that is Verify_Init's; an index out of range takes
// context 0, and k_ed25519_verify_coset_index_mask writes its verdict 0 afterwards
__global__ void __launch_bounds__(ZC_BLOCK) k_ed25519_verify_coset_key_gather(void* pk, const u32* __restrict__ ctxs, size_t n_ctx,
                                                                               const u32* __restrict__ ctx_index, size_t n)
{
    const size_t i = (size_t)blockIdx.x * ZC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 k = ctx_index ? ctx_index[i] : 0u;
    const u32* ctx = ctxs + (size_t)(k < n_ctx ? k : 0u) * VCTX_WORDS;
    u32 w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = ctx[j];
    store32(pk, i, w);
}

__global__ void __launch_bounds__(ZC_BLOCK) k_ed25519_verify_coset_index_mask(int* verdict, const u32* __restrict__ ctx_index, size_t n_ctx, size_t n)
{
    const size_t i = (size_t)blockIdx.x * ZC_BLOCK + threadIdx.x;
    if (i < n && ctx_index[i] >= n_ctx) verdict[i] = 0;
}

namespace {

// what the calling thread's last ed25519_Verify_Check_* call on this device left behind for c25519_amd_verify_check_last_wide:
// 0 (the call never asked), or where its "the two wide combs decide this batch" word lives (the slab's REPORT_WIDE_OK)
thread_local c25519_host::LastCall tl_last_check;

}  // namespace

extern "C" {

// ---- ed25519_Verify_Check_zip215_*: host side (the coset kernels: above) ----------------------------------------------------------------
// The smallest call that walks the contexts (tunable ZIP215_CHECK_MIN; 0 = always): below it the per-lane context kernels lose to
// ed25519_VerifySignature_zip215_dev's per-wave and quad paths on the gathered keys, which give the same verdict for a context that
// is Verify_Init's.  The default is NOT yet set from this call's own cells (tools/verify_check_zip215_rate.py has not been run on a
// device: DESIGN.md, "ZIP-215 against contexts"): it is the smallest size at which the plain pair was measured with the context path
// ahead -- ed25519_Verify_Check_indexed_dev against ed25519_VerifySignature_dev, profiles/indexed_check_rate.txt: 0.82-0.89 x up to
// 2^14, 1.66-1.84 x at 2^16, nothing measured in between -- and both sides of this call run those kernels plus a few percent.
constexpr long ZIP215_CHECK_MIN_DEFAULT = 1L << 16;
static bool zip215_check_walks(size_t n)
{
    const long mn = c25519_host::tunable_or(c25519_host::T_ZIP215_CHECK_MIN, ZIP215_CHECK_MIN_DEFAULT);
    return mn <= 0 || n >= (size_t)mn;
}

// behind a walk that left T in `scr`: coset prep (and rule 2 for the call's contexts, into key_ok), then the shared inversion over the
// prep's products with the coset comparison as its finish
static int launch_coset_finish(const ProjScratch& scr, size_t n, const u32* ctxs, size_t n_ctx, const u32* ctx_index, u32* key_ok,
                               const void* sig, int* verdict, hipStream_t stream)
{
    const unsigned eb = grid_for(n, ZC_BLOCK);
    k_ed25519_verify_coset_prep<<<eb + grid_for(n_ctx, ZC_BLOCK), ZC_BLOCK, 0, stream>>>(scr, n, eb, ctxs, n_ctx, key_ok);
    C25519_TRY(hipGetLastError());
    // This finish keeps more alive per element than the byte comparisons do: with 14 and 16 elements per lane the allocator spilled
    // (34 registers, 656 bytes of scratch per lane), so it is instantiated up to 12 (what 16 buys elsewhere: 9.29 against 9.33 ms per pass)
    const FinishVerifyZip215 fin{ scr.a, scr.b, scr.z, sig, verdict, n, ctx_index, n_ctx, key_ok };
    return launch_invert_k<FinishVerifyZip215, 12>(scr, n, inversion_k(n), fin, stream, scr.prefix);
}

// the keys gathered behind the per-element call's scratch, then that call (ctx_index null: one context)
static int zip215_check_gathered(int* verdict, const void* ctxs, size_t n_ctx, const void* ctx_index, const void* sig, Msgs msgs, size_t n,
                                 hipStream_t stream)
{
    struct Gathered { u32 *inner, *pk; } g;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&g, lease, stream, [n](Carve& c) {
        Gathered s;
        s.inner = inner_verify_scratch(c, n);
        s.pk = c.take(8 * n);                                // the n gathered keys
        return s;
    }));
    k_ed25519_verify_coset_key_gather<<<grid_for(n, ZC_BLOCK), ZC_BLOCK, 0, stream>>>(g.pk, (const u32*)ctxs, n_ctx, (const u32*)ctx_index, n);
    C25519_TRY(hipGetLastError());
    C25519_RC(verify_dev(verdict, sig, g.pk, msgs, n, stream, RULES_ZIP215, /* last_in_call = */ false, g.inner));
    if (ctx_index) {
        k_ed25519_verify_coset_index_mask<<<grid_for(n, ZC_BLOCK), ZC_BLOCK, 0, stream>>>(verdict, (const u32*)ctx_index, n_ctx, n);
        C25519_TRY(hipGetLastError());
    }
    return lease.release();
}

// two-phase verification on the device: contexts are 2080-byte records (pk || 16 x 128-byte canonical rows),
// the reference's EDP_SIGV_CTX size and row order.
int ed25519_Verify_Init_dev(void* ctx, const void* pk, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!ctx || !pk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { ctx, pk })) return rc;
    if (n == 0) return 0;
    if (coop_for(n, 1024))                                  // a few keys: one per wave (which also copies its key into the context)
        k_ed25519_verify_init_coop<<<(unsigned)n, 64, 0, (hipStream_t)stream>>>(pk, n, (u32*)ctx + 8, 2080 / 4, take_done_word(n));
    else {
        C25519_TRY(hipMemcpy2DAsync(ctx, 2080, pk, 32, 32, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        k_ed25519_verify_init<QTableCanon><<<grid_for(n, ED_BLOCK), ED_BLOCK, 0, (hipStream_t)stream>>>(
            pk, n, (u32*)ctx + 8, 2080 / 4);
    }
    C25519_TRY(hipGetLastError());
    return 0;
}

// zip215: ed25519_Verify_Check_zip215_dev above ZIP215_CHECK_MIN -- the same walk (never the per-wave or the quad kernel, which write
// plain verdicts themselves: a remembered comb is walked by the lane kernel at every size), the coset comparison instead of FinishVerify
static int verify_check_one_dev(void* verdict, const void* ctx, const void* sig, const void* msg, size_t msg_size, size_t n,
                                hipStream_t stream, bool zip215)
{
    const Msgs msgs = fixed_msgs(msg, msg_size);
    const u32* tbl = nullptr;
    C25519_RC(base_tables(&tbl, nullptr));
    // a big batch under one key: both scalars over wide combs, if the context is Verify_Init's own and the key is on the
    // curve (k_ed25519_verify_check_wide); decided on the device, the reference-order kernel behind it takes the batch otherwise.
    // Building the key's comb (0.6 ms) pays from ONE_KEY_WIDE signatures per call (2^16); a comb that is REMEMBERED -- one
    // Verify_Init, many Verify_Check calls, ed25519_verify.c:282-286 -- costs nothing, so every call above the per-wave kernels'
    // range asks the device whether its context is the remembered one (one block, 2080 bytes out of L2) and walks the combs if so.
    const long wide_from = c25519_host::tunable_or(c25519_host::T_ONE_KEY_WIDE, 1 << 16);      // (read once per call)
    const bool small = coop_for(n, 1024);
    const bool build = wide_from != 0 && n >= (size_t)wide_from;
    const bool reuse = !build && wide_from != 0 && !small && tls().has_keep();
    const bool try_wide = build || reuse;
    tl_last_check = c25519_host::LastCall::known(0);
    if (!zip215 && !try_wide && small) {                    // a few pairs: one per wave, the reference's order
        k_ed25519_verify_check_coop<<<(unsigned)n, 64, 0, stream>>>((int*)verdict, sig, (const u32*)ctx, msgs, n, tbl, take_done_word(n));
        C25519_TRY(hipGetLastError());
        return 0;
    }
    struct CheckScratch { ProjScratch scr; u32* key_words; } cs;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&cs, lease, stream, [n](Carve& c) {
        CheckScratch s;
        s.scr = c.proj(n);
        s.key_words = c.take(4);                             // four words; the second one is rule 2 for the one context (ZIP-215)
        return s;
    }));
    const ProjScratch& scr = cs.scr;
    u32* wide_ok = nullptr;
    bool quads = false;
    c25519_host::KeepLease keep_lease;                      // records the kept buffer's event however this call leaves
    if (try_wide) {
        const u32* wide_base = nullptr;
        C25519_RC(wide_tables(&wide_base));
        // the key's comb and the context it was built for live in a buffer of the calling thread that outlives the call
        // (ThreadState::keep): the next call with the same context bytes finds them there.  The verdict on THIS call's context
        // (wide_ok) is the call's own: a report word of its work slab (capi_common.hpp: ReportWord), ordered between streams like the
        // slab itself.
        void* keep = nullptr;
        bool fresh = false;
        constexpr size_t KEEP_WORDS = WB_TBL_WORDS + 16 * 32 + KEEP_CTX_WORDS + 1 + 3;
        C25519_RC(keep_lease.acquire(&keep, KEEP_WORDS * sizeof(u32), stream, &fresh));
        u32* wide_key = (u32*)keep;
        u32* check_rows = wide_key + WB_TBL_WORDS;
        u32* remembered = check_rows + 16 * 32;
        C25519_RC(tls().report_word_for(&wide_ok, c25519_host::REPORT_WIDE_OK, stream));
        tl_last_check.reports_in(wide_ok, stream);
        k_ed25519_verify_ctx_prepare<<<build ? 1 + WB_NT * WB_ROWS / 128 : 1, 128, 0, stream>>>(wide_key, check_rows, wide_ok, (const u32*)ctx, remembered, build ? 1 : 0);
        C25519_TRY(hipGetLastError());
        if (build) {
            k_ed25519_verify_ctx_remember<<<1, 128, 0, stream>>>(remembered, (const u32*)ctx, wide_ok);
            C25519_TRY(hipGetLastError());
        }
        quads = !zip215 && one_key_quad_for(n);
        if (quads)                                          // four lanes per pair, the verdict in the same launch
            k_ed25519_verify_check_wide_quad<<<grid_for(n, quad::ELEMS_PER_WAVE), 64, 0, stream>>>(
                (int*)verdict, sig, (const u32*)ctx, msgs, n, wide_base, wide_key, wide_ok);
        else
            k_ed25519_verify_check_wide<<<grid_for(n, WB_BLOCK), WB_BLOCK, 0, stream>>>(
                scr, sig, (const u32*)ctx, msgs, n, wide_base, wide_key, wide_ok);
        C25519_TRY(hipGetLastError());
    }
    k_ed25519_verify_check_shared<<<grid_for(n, ED_BLOCK), ED_BLOCK, 0, stream>>>(
        scr, sig, (const u32*)ctx, msgs, n, tbl, wide_ok);
    C25519_TRY(hipGetLastError());
    if (zip215) {
        C25519_RC(launch_coset_finish(scr, n, (const u32*)ctx, 1, nullptr, cs.key_words + 1, sig, (int*)verdict, stream));
    } else {
        // (the quad kernel has written the verdicts itself where the combs decided: the shared inversion then finds wide_ok set and leaves)
        C25519_RC(launch_invert(scr, n, FinishVerify{ scr.a, scr.b, sig, (int*)verdict, n, quads ? wide_ok : nullptr }, stream));
    }
    C25519_RC(keep_lease.release());
    return lease.release();
}

int ed25519_Verify_Check_dev(void* verdict, const void* ctx, const void* sig, const void* msg, size_t msg_size,
                             size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!verdict || !ctx || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { verdict, ctx, sig })) return rc;
    if (n == 0) return 0;
    return verify_check_one_dev(verdict, ctx, sig, msg, msg_size, n, (hipStream_t)stream_, false);
}

// ed25519_Verify_Check_dev under the strict rules: the plain call, then k_ed25519_verify_check_strict_mask on the same stream
int ed25519_Verify_Check_strict_dev(void* verdict, const void* ctx, const void* sig, const void* msg, size_t msg_size,
                                    size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!verdict || !ctx || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { verdict, ctx, sig })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const DoneWord done = take_done_word(n);               // the mask kernel's, so that the plain kernels find none to signal
    C25519_RC(ed25519_Verify_Check_dev(verdict, ctx, sig, msg, msg_size, n, stream_));
    const unsigned grid = grid_for(n, SM_BLOCK) < SM_MAX_BLOCKS ? grid_for(n, SM_BLOCK) : SM_MAX_BLOCKS;
    k_ed25519_verify_check_strict_mask<<<grid, SM_BLOCK, 0, stream>>>((int*)verdict, sig, n, (const u32*)ctx, done);
    C25519_TRY(hipGetLastError());
    return 0;
}

// n x ed25519_Verify_Check(ctxs + 2080 * ctx_index[i], pair i): up to COOP_MAX pairs (default 1024) one per wave, above that one per
// lane and the shared inversion.  An index >= n_ctx gives verdict 0 (the device cannot refuse the call without a synchronise).
// zip215: ed25519_Verify_Check_zip215_indexed_dev -- below ZIP215_CHECK_MIN the per-element call on the gathered keys; from there
// the lane kernel at every size and the coset comparison instead of FinishVerifyIndexed
static int verify_check_indexed_dev(void* verdict, const void* ctxs, size_t n_ctx, const void* ctx_index, const void* sig, Msgs msgs,
                                    size_t n, hipStream_t stream, bool zip215 = false)
{
    if (int rc = check_dev_args(n, { verdict, ctxs, ctx_index, sig })) return rc;
    if (n == 0) return 0;
    if (n_ctx == 0) return bad_arg("no contexts");
    if (zip215 && !zip215_check_walks(n)) return zip215_check_gathered((int*)verdict, ctxs, n_ctx, ctx_index, sig, msgs, n, stream);
    const u32* tbl = nullptr;
    C25519_RC(base_tables(&tbl, nullptr));
    if (!zip215 && coop_for(n, 1024)) {
        k_ed25519_verify_check_indexed_coop<<<(unsigned)n, 64, 0, stream>>>((int*)verdict, sig, (const u32*)ctxs, n_ctx,
                                                                            (const u32*)ctx_index, msgs, n, tbl, take_done_word(n));
        C25519_TRY(hipGetLastError());
        return 0;
    }
    struct IndexedScratch { u32* rows; ProjScratch scr; u32* key_ok; } is;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&is, lease, stream, [=](Carve& c) {
        IndexedScratch s;
        s.rows = c.take(C25519_INDEXED_REPACK ? n_ctx * QTABLE_CANON_WORDS : 0);   // first in the slab (hipMalloc: 256-byte aligned): whole 128-byte rows
        s.scr = c.proj(n);
        s.key_ok = c.take4(zip215 ? n_ctx : 0);              // rule 2 per context (ZIP-215)
        return s;
    }));
    const auto& [rows, scr, key_ok] = is;
#if C25519_INDEXED_REPACK
    k_ed25519_verify_ctx_repack<<<grid_for(n_ctx * (QTABLE_CANON_WORDS / 4), 256), 256, 0, stream>>>((uint4*)rows, (const u32*)ctxs, n_ctx);
    C25519_TRY(hipGetLastError());
#endif
    k_ed25519_verify_check_indexed<<<grid_for(n, ED_BLOCK), ED_BLOCK, 0, stream>>>(scr, sig, (const u32*)ctxs, n_ctx, (const u32*)ctx_index,
                                                                                  msgs, n, tbl, rows);
    C25519_TRY(hipGetLastError());
    if (zip215)
        C25519_RC(launch_coset_finish(scr, n, (const u32*)ctxs, n_ctx, (const u32*)ctx_index, key_ok, sig, (int*)verdict, stream));
    else
        C25519_RC(launch_invert(scr, n, FinishVerifyIndexed{ scr.a, scr.b, sig, (int*)verdict, n, (const u32*)ctx_index, n_ctx }, stream));
    return lease.release();
}

int ed25519_Verify_Check_indexed_dev(void* verdict, const void* ctxs, size_t n_ctx, const void* ctx_index, const void* sig,
                                     const void* msg, size_t msg_size, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !ctxs || !ctx_index || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    return verify_check_indexed_dev(verdict, ctxs, n_ctx, ctx_index, sig, fixed_msgs(msg, msg_size), n, (hipStream_t)stream);
}

int ed25519_Verify_Check_indexed_ragged_dev(void* verdict, const void* ctxs, size_t n_ctx, const void* ctx_index, const void* sig,
                                            const void* msgs, const uint64_t* offsets, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !ctxs || !ctx_index || !sig || !offsets) return bad_arg("null pointer");
    return verify_check_indexed_dev(verdict, ctxs, n_ctx, ctx_index, sig, ragged_msgs(msgs, offsets), n, (hipStream_t)stream);
}

// the ZIP-215 verdict against contexts (include/curve25519_amd.h): arguments and argument errors of the plain calls they are named after
int ed25519_Verify_Check_zip215_dev(void* verdict, const void* ctx, const void* sig, const void* msg, size_t msg_size,
                                    size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!verdict || !ctx || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { verdict, ctx, sig })) return rc;
    if (n == 0) return 0;
    if (!zip215_check_walks(n)) {
        tl_last_check = c25519_host::LastCall::known(0);
        return zip215_check_gathered((int*)verdict, ctx, 1, nullptr, sig, fixed_msgs(msg, msg_size), n, (hipStream_t)stream_);
    }
    return verify_check_one_dev(verdict, ctx, sig, msg, msg_size, n, (hipStream_t)stream_, true);
}

int ed25519_Verify_Check_zip215_indexed_dev(void* verdict, const void* ctxs, size_t n_ctx, const void* ctx_index, const void* sig,
                                            const void* msg, size_t msg_size, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !ctxs || !ctx_index || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    return verify_check_indexed_dev(verdict, ctxs, n_ctx, ctx_index, sig, fixed_msgs(msg, msg_size), n, (hipStream_t)stream, true);
}

int ed25519_Verify_Check_zip215_indexed_ragged_dev(void* verdict, const void* ctxs, size_t n_ctx, const void* ctx_index, const void* sig,
                                                   const void* msgs, const uint64_t* offsets, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !ctxs || !ctx_index || !sig || !offsets) return bad_arg("null pointer");
    return verify_check_indexed_dev(verdict, ctxs, n_ctx, ctx_index, sig, ragged_msgs(msgs, offsets), n, (hipStream_t)stream, true);
}

// test / accounting hook: did the calling thread's last ed25519_Verify_Check_* call on this device walk the two wide combs (1), or
// did the reference-order kernel decide it (0: the call did not ask -- too small, no remembered comb, ONE_KEY_WIDE = 0 -- or the
// device said no: another context than the remembered one, a context that is not Verify_Init's, an off-curve key)?  -1: no such
// call to report.  Synchronises with that call's stream.  (A *_batch call of several pieces reports its last piece.)
long c25519_amd_verify_check_last_wide(void)
{
    C25519_API_CALL_OR(-1);
    const long v = tl_last_check.read();
    return v > 0 ? 1 : v;
}

}  // extern "C"
