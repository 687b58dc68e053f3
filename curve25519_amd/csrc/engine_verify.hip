// curve25519_amd/csrc/engine_verify.hip -- Ed25519 verification: the lattice path (scalars, points, walk; on quads; one launch of three waves), the
// reference order, the two-phase calls with one key (shared table, two wide combs), key classification and conversion to X25519 keys --
// kernels and *_dev entry points
// (one of the engine's four translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "verify_ctx.cuh"
#include "verify_ctx_zip215.cuh"
#include "ed_keys.cuh"

// ed25519_Verify_Init (ed25519_verify.c:179-232): decompress -A (inverted parity :192-195, no validation) and
// fill the key's 16-row 4-fold table.  `tables` holds n tables of Tbl's format, `stride_words` apart.
template <typename Tbl>
__global__ void __launch_bounds__(ED_BLOCK, C25519_VI_WAVES) k_ed25519_verify_init(const void* pk, size_t n, u32* tables,
                                                                      size_t stride_words)
{
    const size_t i = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pkw[8];
    load32(pkw, pk, i);
    ge_ext Q;
    ed_decode_neg_key(Q, pkw);
    const Tbl tbl{ tables + i * stride_words };
    qtable_build(tbl, Q);
}

// ed25519_Verify_Check (ed25519_verify.c:287-313), first part: h = H(enc(R) || pk || m) mod L canonical;
// s = raw 256 bits (no s < L check, :308); T = s*B + h*(-A) projective.  The comparison with enc(R) happens in
// k_batch_invert<FinishVerify>.
template <typename Tbl>
C25519_DEV void verify_check_lane(const ProjScratch& scr, size_t n, size_t i, const void* sig, const u32 (&pkw)[8],
                                  const Msgs& msgs, const Tbl& tbl, const u32* lds_tbl)
{
    u32 Sw[8], h[8], Rw[8];
    load32(Rw, sig, 2 * i);
    ed_hram(h, Rw, pkw, msgs.ptr(i), msgs.len(i));
    sc_mod(h);
    load32(Sw, sig, 2 * i + 1);
    ge_ext T;
    ge_poly_mult(T, Sw, h, tbl, lds_tbl);
    store_proj(scr, n, i, T);
}

template <typename Tbl>
__global__ void __launch_bounds__(ED_BLOCK, C25519_VC_WAVES) k_ed25519_verify_check(ProjScratch scr, const void* sig, const void* pk,
                                                                       Msgs msgs, size_t n,
                                                                       const u32* __restrict__ g_tbl, u32* tables,
                                                                       size_t stride_words)
{
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[PA_WORDS * 256];
    lds_stage_words(lds_tbl, g_tbl + REF_TBL_OFFSET, REF_TBL_WORDS);
    const size_t i = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pkw[8];
    load32(pkw, pk, i);
    const Tbl tbl{ tables + i * stride_words };
    verify_check_lane(scr, n, i, sig, pkw, msgs, tbl, lds_tbl);
}

// ---- the lattice fast path (verify_fast.cuh) ---------------------------------------------------------------------------
// Four kernels.  scalars -> points -> walk decide every element whose key is on the curve (and whose short
// vector fits the walk: a random one practically always does); the elements they cannot decide are collected in a list
// and k_ed25519_verify_slow runs the reference's own operation order for exactly those.
// Per-element hand-over, struct-of-arrays: sigma_cols[SIGMA_WORDS] (sigma's signed comb columns), rho[5], tau[5] (biased), a flag word
//   bit 0  R decodes canonically onto the curve      bit 1  the key is on the curve
//   bit 2  the short vector fits the walk             bit 3  tau < 0
//   bit 4  the element is on the slow list            bit 5  the element breaks a strict input rule (strict calls only)
//   bits 8..13  top nonzero digit of the element's scalars
// (FastScratch, the scratch of the lattice path, and the FLAG_* bits: coop_ops.cuh)
constexpr int FS_BLOCK = 256;
#ifndef C25519_VW_WAVES
#define C25519_VW_WAVES 2            // waves per SIMD the register allocator aims at: the walk kernel (rows prefetched) ...
#endif
#ifndef C25519_WALK_BLOCK
#define C25519_WALK_BLOCK C25519_ED_BLOCK       // lanes per walk workgroup (they share one staged comb table)
#endif
constexpr int WALK_BLOCK = C25519_WALK_BLOCK;
#ifndef C25519_VD_WAVES
#define C25519_VD_WAVES 3            // ... and the point decoding + table kernel
#endif

// Strict (the kernels' *_strict twins): rules 1 and 5 here, rules 2-4 in the key lane of the points, which writes verdict 0 for a
// rejected element and marks it FLAG_REJECT | FLAG_SLOW: the plain walk skips it, and it goes on no list
template <bool Strict = false>
C25519_DEV void verify_scalars_lane(const FastScratch& fs, const void* sig, const void* pk, const Msgs& msgs, size_t n, size_t i)
{
    u32 pkw[8], Rw[8], Sw[8], cols[SIGMA_WORDS], rho[5], tau[5], tau_neg;
    load32(pkw, pk, i);
    load32(Rw, sig, 2 * i);
    load32(Sw, sig, 2 * i + 1);
    const u32 lat_ok = ed_verify_fast_scalars(cols, rho, tau, tau_neg, pkw, Rw, Sw, msgs.ptr(i), msgs.len(i), fs.lat_cap_bits);
#pragma unroll
    for (int w = 0; w < SIGMA_WORDS; w++) fs.sigma[(size_t)w * n + i] = cols[w];
#pragma unroll
    for (int w = 0; w < 5; w++) { fs.rho[(size_t)w * n + i] = rho[w]; fs.tau[(size_t)w * n + i] = tau[w]; }
    const int top = lat_ok ? walk_top_digit(tau, rho) : 0;
    if (Strict) {                                            // R and S again from L2: kept across the hash they cost a wave per SIMD
        load32(Rw, sig, 2 * i);
        load32(Sw, sig, 2 * i + 1);
        fs.flags[i] = (lat_ok & FLAG_FITS) | (tau_neg & FLAG_TAU_NEG) | ((u32)top << 8) | strict_pair_flags(Rw, Sw);
    } else
        fs.flags[i] = (lat_ok & FLAG_FITS) | (tau_neg & FLAG_TAU_NEG) | ((u32)top << 8);
}


// step 1: hash, short lattice vector, sigma -- integer work only
template <bool Strict>
C25519_DEV void verify_fast_scalars(const FastScratch& fs, const void* sig, const void* pk, const Msgs& msgs, size_t n)
{
    const size_t i = (size_t)blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i == 0) fs.slow_count[0] = fs.slow_count[1] = fs.slow_count[2] = 0;
    if (i >= n) return;
    verify_scalars_lane<Strict>(fs, sig, pk, msgs, n, i);
}

__global__ void __launch_bounds__(FS_BLOCK) k_ed25519_verify_fast_scalars(FastScratch fs, const void* sig, const void* pk,
                                                                          Msgs msgs, size_t n)
{
    verify_fast_scalars<false>(fs, sig, pk, msgs, n);
}

__global__ void __launch_bounds__(FS_BLOCK) k_ed25519_verify_fast_scalars_strict(FastScratch fs, const void* sig, const void* pk,
                                                                                 Msgs msgs, size_t n)
{
    verify_fast_scalars<true>(fs, sig, pk, msgs, n);
}

// step 2: the two points of an element, one per lane: lane j < n decodes key j, lane n + j decodes R of signature j (a
// square root each), then builds that point's window table.  2n lanes, 168 registers: three waves per SIMD, no spills.
template <bool Strict>
C25519_DEV void verify_fast_points(FastScratch fs, const void* sig, const void* pk, size_t n, int* verdict)
{
    const size_t j = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (j >= 2 * n) return;
    const bool is_r = j >= n;
    const size_t e = is_r ? j - n : j;
    u32 w[8];
    if (is_r) load32(w, sig, 2 * e); else load32(w, pk, e);
    const u32 f = fs.flags[e];
    const u32 tau_neg = (f & FLAG_TAU_NEG) ? 0xffffffffu : 0u;
    fe X, Y;
    const u32 ok = ed_verify_fast_decode(X, Y, w, is_r ? 0xffffffffu : 0u, tau_neg) & (Strict && !is_r ? ~strict_reject_key(w) : 0xffffffffu);
    if (!is_r) {                                                   // the walk's order (see FastScratch::order)
        const bool is_long = ((f >> 8) & 63u) > 32u;
        const u32 pos = is_long ? (u32)n - 1u - atomicAdd(fs.slow_count + 2, 1u) : atomicAdd(fs.slow_count + 1, 1u);
        fs.order[pos] = (u32)e;
    }
    if (is_r) {
        if (ok) atomicOr(&fs.flags[e], FLAG_R_OK);
    } else if (Strict) {
        // strict_key_flags (coop_ops.cuh): a rejected element is marked as listed, so that the plain walk skips it, but goes on no list;
        // its verdict is written here
        const u32 add = strict_key_flags(f, ok);
        atomicOr(&fs.flags[e], add);
        if (add & FLAG_REJECT) verdict[e] = 0;
        else if (add & FLAG_SLOW) fs.slow_list[atomicAdd(fs.slow_count, 1u)] = (u32)e;
    } else if (ok && (f & FLAG_FITS)) {
        atomicOr(&fs.flags[e], FLAG_KEY_OK);
    } else {                                                      // an element the walk cannot decide: on the slow list
        atomicOr(&fs.flags[e], ok ? FLAG_KEY_OK | FLAG_SLOW : FLAG_SLOW);
        fs.slow_list[atomicAdd(fs.slow_count, 1u)] = (u32)e;      // (the compiler aggregates this per wave)
    }
    // the point's window table, right here: a table is 1152 bytes of 16-byte stores scattered over as many cache lines, and
    // they hide under the other waves' square roots (measured with the earlier 160-byte rows: in a kernel of their own 1.3 ms
    // with the SIMDs idle half the time; in front of the walk, inside its kernel, 1.0 ms; here 0.6 ms --
    // profiles/r03_ab_verify_structure.txt).
    // (An element that turns out to be on the slow list gets tables nobody reads: the key lane cannot tell the R lane in time.)
    wtable_build(fs.tables + e * FAST_TABLE_WORDS + (is_r ? WTABLE_WORDS : 0), X, Y);
}

__global__ void __launch_bounds__(ED_BLOCK, C25519_VD_WAVES) k_ed25519_verify_fast_points(FastScratch fs, const void* sig, const void* pk,
                                                                                          size_t n)
{
    verify_fast_points<false>(fs, sig, pk, n, nullptr);
}

__global__ void __launch_bounds__(ED_BLOCK, C25519_VD_WAVES) k_ed25519_verify_fast_points_strict(FastScratch fs, const void* sig,
                                                                                                 const void* pk, size_t n, int* verdict)
{
    verify_fast_points<true>(fs, sig, pk, n, verdict);
}

// step 3: the walk and the neutral-element test (ge_walk_is_neutral).  Beside the accumulator point only the round's two
// packed table rows live in registers -- fetched at the top of the round, unpacked field by field when the additions want
// them -- ; the scalars are fetched a word at a time, LDS rows a field at a time: 216 registers, two waves per SIMD, no
// spills.  The kernel is VALU-bound: a SIMD has a VALU instruction executing in 97 % of the shader's cycles
// (SQ_ACTIVE_INST_VALU * 4 / 1024 against GRBM_GUI_ACTIVE / 8, profiles/r03_pmc.txt), and it measured the same at two,
// three (154 registers without the prefetch) and four waves per SIMD.
__global__ void __launch_bounds__(WALK_BLOCK, C25519_VW_WAVES) k_ed25519_verify_fast_walk(FastScratch fs, int* verdict, size_t n,
                                                                                        const u32* __restrict__ g_tbl)
{
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[SC_TBL_WORDS];
    lds_stage_words(lds_tbl, g_tbl + SC_TBL_OFFSET, SC_TBL_WORDS);
    const size_t lane = (size_t)blockIdx.x * WALK_BLOCK + threadIdx.x;
    const size_t i = lane < n ? fs.order[lane] : n;      // (lane j taking element j lost: profiles/r03_ab_verify_structure.txt block 14)
    const u32 f = i < n ? fs.flags[i] : FLAG_SLOW;
    const bool walks = !(f & FLAG_SLOW);
    // the wave walks from its longest element's first digit (the others' digits above their own are zero)
    int top = walks ? (int)((f >> 8) & 63u) : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(top, o);
        top = other > top ? other : top;
    }
    top = __builtin_amdgcn_readfirstlane(top);           // wave-uniform by construction: let the walk's loops be scalar ones
    if (!walks) return;
    const u32* tq = fs.tables + i * FAST_TABLE_WORDS;
    const WalkScalars sc{ fs.sigma, fs.tau, fs.rho, n, i };
    const u32 neutral = ge_walk_is_neutral(sc, tq, tq + WTABLE_WORDS, lds_tbl, top < 8 ? 8 : top);
    verdict[i] = (neutral & f & FLAG_R_OK) ? 1 : 0;
}

// Batches of 2^11 .. 2^15 signatures leave most of the chip idle under one-lane kernels (2^14 elements: 256 waves on 1024 SIMDs), so
// their path is shaped for the LENGTH of the chain, not for instructions per element:
//  * k_ed25519_verify_quad_prep -- ONE launch for steps 1 and 2: the first workgroups hash and reduce (50 us), the others decode the
//    two points of every element and build their window tables (92 us) AT THE SAME TIME.  The points cannot know tau's sign yet:
//    they tabulate the key as decoded, and the walk flips the rows' signs where tau < 0.  Each lane reports its point in a word of
//    its own (pflags), so nothing here is ordered against the scalar workgroups.
//  * k_ed25519_verify_quad_walk -- step 3 on QUADS (quad25519.cuh: quad::walk_is_neutral): four lanes per element walk an addition
//    in two product levels and a doubling in a level of squarings and one of products (~2.3 x shorter than a lane's); it also
//    makes the slow list (an element the walk cannot decide: off-curve key, over-long vector) for step 5 behind it.  64 elements
//    (four waves) per workgroup share one staged comb table; element order (no long / short sorting: 16 elements per wave).
//  * Strict (the *_strict twins): the scalar lanes apply rules 1 and 5, a key lane rules 2-4 (its pflags word is then zero); the walk
//    writes verdict 0 for an element that breaks one, and lists it nowhere.  The two twins are written out: as templates of the plain
//    kernels they changed the plain kernels' gfx950 code (instruction order), which must stay what it was.
__global__ void __launch_bounds__(ED_BLOCK, C25519_VD_WAVES) k_ed25519_verify_quad_prep(FastScratch fs, const void* sig, const void* pk,
                                                                                         Msgs msgs, size_t n, unsigned scalar_blocks)
{
    static_assert(FS_BLOCK == ED_BLOCK, "one workgroup shape for both roles");
    if (blockIdx.x < scalar_blocks) {
        const size_t i = (size_t)blockIdx.x * FS_BLOCK + threadIdx.x;
        if (i == 0) fs.slow_count[0] = fs.slow_count[1] = fs.slow_count[2] = 0;
        if (i >= n) return;
        verify_scalars_lane(fs, sig, pk, msgs, n, i);
        return;
    }
    const size_t j = (size_t)(blockIdx.x - scalar_blocks) * ED_BLOCK + threadIdx.x;
    if (j >= 2 * n) return;
    const bool is_r = j >= n;
    const size_t e = is_r ? j - n : j;
    u32 w[8];
    if (is_r) load32(w, sig, 2 * e); else load32(w, pk, e);
    fe X, Y;
    const u32 ok = ed_verify_fast_decode(X, Y, w, is_r ? 0xffffffffu : 0u, 0u);
    fs.pflags[j] = ok;
    wtable_build(fs.tables + e * FAST_TABLE_WORDS + (is_r ? WTABLE_WORDS : 0), X, Y);
}

__global__ void __launch_bounds__(ED_BLOCK, C25519_VD_WAVES) k_ed25519_verify_quad_prep_strict(FastScratch fs, const void* sig, const void* pk,
                                                                                                Msgs msgs, size_t n, unsigned scalar_blocks)
{
    if (blockIdx.x < scalar_blocks) {
        const size_t i = (size_t)blockIdx.x * FS_BLOCK + threadIdx.x;
        if (i == 0) fs.slow_count[0] = fs.slow_count[1] = fs.slow_count[2] = 0;
        if (i >= n) return;
        verify_scalars_lane<true>(fs, sig, pk, msgs, n, i);
        return;
    }
    const size_t j = (size_t)(blockIdx.x - scalar_blocks) * ED_BLOCK + threadIdx.x;
    if (j >= 2 * n) return;
    const bool is_r = j >= n;
    const size_t e = is_r ? j - n : j;
    u32 w[8];
    if (is_r) load32(w, sig, 2 * e); else load32(w, pk, e);
    fe X, Y;
    const u32 ok = ed_verify_fast_decode(X, Y, w, is_r ? 0xffffffffu : 0u, 0u) & (is_r ? 0xffffffffu : ~strict_reject_key(w));
    fs.pflags[j] = ok;
    wtable_build(fs.tables + e * FAST_TABLE_WORDS + (is_r ? WTABLE_WORDS : 0), X, Y);
}

constexpr int QW_BLOCK = 256;
__global__ void __launch_bounds__(QW_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_ed25519_verify_quad_walk(FastScratch fs, int* verdict, size_t n, const u32* __restrict__ g_tbl)
{
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[SC_TBL_WORDS];
    lds_stage_words(lds_tbl, g_tbl + SC_TBL_OFFSET, SC_TBL_WORDS);
    const size_t i = (size_t)blockIdx.x * (QW_BLOCK / 4) + (threadIdx.x >> 2);
    const u32 f = i < n ? fs.flags[i] : 0u;
    const u32 key_ok = i < n ? fs.pflags[i] : 0u, r_ok = i < n ? fs.pflags[n + i] : 0u;
    const bool walks = (f & FLAG_FITS) && key_ok;
    int top = walks ? (int)((f >> 8) & 63u) : 0;           // the wave walks from its longest element's first digit
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(top, o);
        top = other > top ? other : top;
    }
    top = __builtin_amdgcn_readfirstlane(top);
    const quad::Roles R = quad::roles();
    if (!walks) {                                         // (whole quads leave)
        if (i < n && R.is0) fs.slow_list[atomicAdd(fs.slow_count, 1u)] = (u32)i;
        return;
    }
    const u32* tq = fs.tables + i * FAST_TABLE_WORDS;
    const WalkScalars sc{ fs.sigma, fs.tau, fs.rho, n, i };
    const u32 q_flip = (f & FLAG_TAU_NEG) ? 0xffffffffu : 0u;
    const u32 neutral = quad::walk_is_neutral(sc, tq, tq + WTABLE_WORDS, lds_tbl, top < 8 ? 8 : top, R, q_flip);
    if (R.is0) verdict[i] = (neutral & r_ok) ? 1 : 0;
}

// ... the strict twin (a key that breaks rules 2-4 has pflags 0: it is rejected, not listed)
__global__ void __launch_bounds__(QW_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_ed25519_verify_quad_walk_strict(FastScratch fs, int* verdict, size_t n, const u32* __restrict__ g_tbl)
{
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[SC_TBL_WORDS];
    lds_stage_words(lds_tbl, g_tbl + SC_TBL_OFFSET, SC_TBL_WORDS);
    const size_t i = (size_t)blockIdx.x * (QW_BLOCK / 4) + (threadIdx.x >> 2);
    const u32 f = i < n ? fs.flags[i] : 0u;
    const u32 key_ok = i < n ? fs.pflags[i] : 0u, r_ok = i < n ? fs.pflags[n + i] : 0u;
    const bool rejected = i < n && ((f & FLAG_REJECT) || !key_ok);
    const bool walks = !rejected && (f & FLAG_FITS);
    int top = walks ? (int)((f >> 8) & 63u) : 0;           // the wave walks from its longest element's first digit
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(top, o);
        top = other > top ? other : top;
    }
    top = __builtin_amdgcn_readfirstlane(top);
    const quad::Roles R = quad::roles();
    if (!walks) {                                         // (whole quads leave)
        if (rejected && R.is0) verdict[i] = 0;
        else if (i < n && R.is0) fs.slow_list[atomicAdd(fs.slow_count, 1u)] = (u32)i;
        return;
    }
    const u32* tq = fs.tables + i * FAST_TABLE_WORDS;
    const WalkScalars sc{ fs.sigma, fs.tau, fs.rho, n, i };
    const u32 q_flip = (f & FLAG_TAU_NEG) ? 0xffffffffu : 0u;
    const u32 neutral = quad::walk_is_neutral(sc, tq, tq + WTABLE_WORDS, lds_tbl, top < 8 ? 8 : top, R, q_flip);
    if (R.is0) verdict[i] = (neutral & r_ok) ? 1 : 0;
}

// The whole lattice path of ONE element in ONE launch, for a call of a few elements: a workgroup of THREE waves per element
// (coop::verify_three_waves, coop_ops.cuh: wave 0 hashes and reduces while wave 1 takes the two square roots; then the three
// products of sigma*B + tau*Q + rho*(-R) = O side by side, a wave each; wave 0 adds and tests).  Three launches ran
// 40 + 83 + 91 us one after the other for one signature; this is ~60 + ~60.  The host zeroes the slow list's counter in front
// of the launch.
__global__ void __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_ed25519_verify_one_per_group(FastScratch fs, int* verdict, const void* sig, const void* pk, Msgs msgs, size_t n,
                               const u32* __restrict__ g_tbl)
{
    __shared__ __attribute__((aligned(16))) u32 lds_all[coop::V3_LDS_WORDS];
    __shared__ u32 park[40], hand[4];
    if (blockIdx.x >= n) return;
    coop::verify_three_waves(lds_all, park, hand, fs, verdict, sig, pk, msgs, n, blockIdx.x, g_tbl);
}

__global__ void __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_ed25519_verify_one_per_group_strict(FastScratch fs, int* verdict, const void* sig, const void* pk, Msgs msgs, size_t n,
                                      const u32* __restrict__ g_tbl)
{
    __shared__ __attribute__((aligned(16))) u32 lds_all[coop::V3_LDS_WORDS];
    __shared__ u32 park[40], hand[4];
    if (blockIdx.x >= n) return;
    coop::verify_three_waves<true>(lds_all, park, hand, fs, verdict, sig, pk, msgs, n, blockIdx.x, g_tbl);
}

// step 5: the elements on the slow list (off-curve keys -- the reference does not reject them, so neither may we -- and
// the practically nonexistent over-long vectors), one per lane, in the reference's order (ed_verify_reference_order),
// behind the walk on the same stream.  The grid covers the worst case (every element listed); workgroups beyond the
// list's end read the counter and leave: with honest keys that is all of them and costs ~10 us.  A batch with garbage keys
// in it pays one reference-order verification's latency (~1.3 ms) on top.
// (Tried and dropped: the kernel on a second, high-priority stream beside the walk -- its workgroups only ever found room
// when the walk's last round drained, profiles/r03_ab_verify_structure.txt; a fixed small grid striding over the list --
// any loop around the body makes the compiler keep ~60 field constants in registers across trips: 268 instead of 200.)
__global__ void __launch_bounds__(ED_BLOCK, 2) k_ed25519_verify_slow(FastScratch fs, int* verdict, const void* sig, const void* pk,
                                                                     Msgs msgs, const u32* __restrict__ g_tbl, DoneWord done)
{
    // done: a call of ONE element only (its list holds at most that element, which thread 0 of block 0 then decides)
    const u32 count = *fs.slow_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *fs.slow_report = count;
        if (count == 0) signal_done(done);
    }
    if ((size_t)blockIdx.x * ED_BLOCK >= count) return;
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[PA_WORDS * 256];
    lds_stage_words(lds_tbl, g_tbl + REF_TBL_OFFSET, REF_TBL_WORDS);
    const size_t k = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (k >= count) return;
    const size_t i = fs.slow_list[k];
    u32 pkw[8], Rw[8], Sw[8];
    load32(pkw, pk, i);
    load32(Rw, sig, 2 * i);
    load32(Sw, sig, 2 * i + 1);
    verdict[i] = ed_verify_reference_order(pkw, Rw, Sw, msgs.ptr(i), msgs.len(i), fs.tables + i * FAST_TABLE_WORDS, lds_tbl);
    if (k == 0) signal_done(done);
}

// Same check with ONE key for the whole batch (the reference's two-phase use: Verify_Init once, many
// Verify_Check calls, ed25519_verify.c:282-286).  ctx is the 2080-byte context (pk || 16 canonical rows); the
// workgroup converts it once into limb form in LDS (limb-major, 16 rows wide: the 16 possible row indices
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

// ---- ed25519_VerifySignature_zip215_*: the lattice path under the ZIP-215 rule ---------------------------------------------------------
// Twins of the lattice path's kernels, written out and kept behind them (as templates of the plain kernels, or in between them, they
// changed the plain kernels' gfx950 code, which must stay what it was).  The walk computes W = [rho](S*B - k*A - R) with rho odd:
// multiplication by rho permutes the 8-torsion, so [8]W = O is the rule's equation.  The quad and per-wave walks double W three times
// in front of the neutral test.  The lane path has no walk of its own -- any twin of k_ed25519_verify_fast_walk changed that kernel's
// code -- and hands the plain walk scalars multiplied by 8 instead (ed_verify_zip215_scalars), at 0.75 digit rounds per wave.
// S >= L (FLAG_REJECT from the scalar step) and a key without a square root get verdict 0 where the key is decoded and go on no list;
// an R without one gets 0 from the walk or the fallback.  The slow list holds over-long vectors only, and its kernel is cofactored too.
template <bool Scale8>
C25519_DEV void verify_scalars_lane_zip215(const FastScratch& fs, const void* sig, const void* pk, const Msgs& msgs, size_t n, size_t i)
{
    u32 pkw[8], Rw[8], Sw[8], cols[SIGMA_WORDS], rho[5], tau[5], tau_neg;
    load32(pkw, pk, i);
    load32(Rw, sig, 2 * i);
    load32(Sw, sig, 2 * i + 1);
    const u32 lat_ok = ed_verify_zip215_scalars(cols, rho, tau, tau_neg, pkw, Rw, Sw, msgs.ptr(i), msgs.len(i), fs.lat_cap_bits, Scale8);
#pragma unroll
    for (int w = 0; w < SIGMA_WORDS; w++) fs.sigma[(size_t)w * n + i] = cols[w];
#pragma unroll
    for (int w = 0; w < 5; w++) { fs.rho[(size_t)w * n + i] = rho[w]; fs.tau[(size_t)w * n + i] = tau[w]; }
    const int top = lat_ok ? walk_top_digit(tau, rho) : 0;
    load32(Sw, sig, 2 * i + 1);                              // S again from L2, as the strict lane does
    fs.flags[i] = (lat_ok & FLAG_FITS) | (tau_neg & FLAG_TAU_NEG) | ((u32)top << 8) | zip215_pair_flags(Sw);
}

__global__ void __launch_bounds__(FS_BLOCK) k_ed25519_verify_fast_scalars_zip215(FastScratch fs, const void* sig, const void* pk,
                                                                                 Msgs msgs, size_t n)
{
    const size_t i = (size_t)blockIdx.x * FS_BLOCK + threadIdx.x;
    if (i == 0) fs.slow_count[0] = fs.slow_count[1] = fs.slow_count[2] = 0;
    if (i >= n) return;
    verify_scalars_lane_zip215<true>(fs, sig, pk, msgs, n, i);   // scalars times 8: the plain walk kernel then tests [8]W
}

// k_ed25519_verify_fast_points under the ZIP-215 rule: both points by ed_zip215_decode (no canonical-encoding term).  A key without a square root, or an
// element with S >= L, gets verdict 0 here and is marked as listed without being listed; an R without one leaves FLAG_R_OK clear
// (the walk, or the fallback for an over-long vector, then answers 0).
__global__ void __launch_bounds__(ED_BLOCK, C25519_VD_WAVES) k_ed25519_verify_fast_points_zip215(FastScratch fs, const void* sig,
                                                                                                 const void* pk, size_t n, int* verdict)
{
    const size_t j = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (j >= 2 * n) return;
    const bool is_r = j >= n;
    const size_t e = is_r ? j - n : j;
    u32 w[8];
    if (is_r) load32(w, sig, 2 * e); else load32(w, pk, e);
    const u32 f = fs.flags[e];
    fe X, Y;
    const u32 ok = ed_zip215_decode(X, Y, w, (is_r || !(f & FLAG_TAU_NEG)) ? 0xffffffffu : 0u);
    if (!is_r) {                                                   // the walk's order (see FastScratch::order)
        const bool is_long = ((f >> 8) & 63u) > 33u;               // (scalars times 8: a digit later than the plain kernel's split)
        const u32 pos = is_long ? (u32)n - 1u - atomicAdd(fs.slow_count + 2, 1u) : atomicAdd(fs.slow_count + 1, 1u);
        fs.order[pos] = (u32)e;
    }
    if (is_r) {
        if (ok) atomicOr(&fs.flags[e], FLAG_R_OK);
    } else {
        const u32 add = strict_key_flags(f, ok);
        atomicOr(&fs.flags[e], add);
        if (add & FLAG_REJECT) verdict[e] = 0;
        else if (add & FLAG_SLOW) fs.slow_list[atomicAdd(fs.slow_count, 1u)] = (u32)e;
    }
    wtable_build(fs.tables + e * FAST_TABLE_WORDS + (is_r ? WTABLE_WORDS : 0), X, Y);
}

// k_ed25519_verify_quad_prep: rule 1 in the scalar lanes, both points by ed_zip215_decode as decoded (the walk flips the key's rows)
__global__ void __launch_bounds__(ED_BLOCK, C25519_VD_WAVES) k_ed25519_verify_quad_prep_zip215(FastScratch fs, const void* sig, const void* pk,
                                                                                                Msgs msgs, size_t n, unsigned scalar_blocks)
{
    if (blockIdx.x < scalar_blocks) {
        const size_t i = (size_t)blockIdx.x * FS_BLOCK + threadIdx.x;
        if (i == 0) fs.slow_count[0] = fs.slow_count[1] = fs.slow_count[2] = 0;
        if (i >= n) return;
        verify_scalars_lane_zip215<false>(fs, sig, pk, msgs, n, i);
        return;
    }
    const size_t j = (size_t)(blockIdx.x - scalar_blocks) * ED_BLOCK + threadIdx.x;
    if (j >= 2 * n) return;
    const bool is_r = j >= n;
    const size_t e = is_r ? j - n : j;
    u32 w[8];
    if (is_r) load32(w, sig, 2 * e); else load32(w, pk, e);
    fe X, Y;
    const u32 ok = ed_zip215_decode(X, Y, w, 0xffffffffu);      // -A (tau's sign is not known yet) and -R
    fs.pflags[j] = ok;
    wtable_build(fs.tables + e * FAST_TABLE_WORDS + (is_r ? WTABLE_WORDS : 0), X, Y);
}

// k_ed25519_verify_quad_walk: S >= L, a key or an R without a square root: verdict 0, listed nowhere; [8]W in front of the neutral test
__global__ void __launch_bounds__(QW_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_ed25519_verify_quad_walk_zip215(FastScratch fs, int* verdict, size_t n, const u32* __restrict__ g_tbl)
{
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[SC_TBL_WORDS];
    lds_stage_words(lds_tbl, g_tbl + SC_TBL_OFFSET, SC_TBL_WORDS);
    const size_t i = (size_t)blockIdx.x * (QW_BLOCK / 4) + (threadIdx.x >> 2);
    const u32 f = i < n ? fs.flags[i] : 0u;
    const u32 key_ok = i < n ? fs.pflags[i] : 0u, r_ok = i < n ? fs.pflags[n + i] : 0u;
    const bool rejected = i < n && ((f & FLAG_REJECT) || !key_ok || !r_ok);
    const bool walks = !rejected && (f & FLAG_FITS);
    int top = walks ? (int)((f >> 8) & 63u) : 0;           // the wave walks from its longest element's first digit
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int other = __shfl_xor(top, o);
        top = other > top ? other : top;
    }
    top = __builtin_amdgcn_readfirstlane(top);
    const quad::Roles R = quad::roles();
    if (!walks) {                                         // (whole quads leave)
        if (rejected && R.is0) verdict[i] = 0;
        else if (i < n && R.is0) fs.slow_list[atomicAdd(fs.slow_count, 1u)] = (u32)i;
        return;
    }
    const u32* tq = fs.tables + i * FAST_TABLE_WORDS;
    const WalkScalars sc{ fs.sigma, fs.tau, fs.rho, n, i };
    const u32 q_flip = (f & FLAG_TAU_NEG) ? 0xffffffffu : 0u;
    const u32 neutral = quad::walk_is_neutral<true>(sc, tq, tq + WTABLE_WORDS, lds_tbl, top < 8 ? 8 : top, R, q_flip);
    if (R.is0) verdict[i] = neutral ? 1 : 0;
}

// k_ed25519_verify_one_per_group: coop::verify_three_waves in its ZIP-215 form
__global__ void __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_ed25519_verify_one_per_group_zip215(FastScratch fs, int* verdict, const void* sig, const void* pk, Msgs msgs, size_t n,
                                      const u32* __restrict__ g_tbl)
{
    __shared__ __attribute__((aligned(16))) u32 lds_all[coop::V3_LDS_WORDS];
    __shared__ u32 park[40], hand[4];
    if (blockIdx.x >= n) return;
    coop::verify_three_waves<false, true>(lds_all, park, hand, fs, verdict, sig, pk, msgs, n, blockIdx.x, g_tbl);
}

// k_ed25519_verify_slow: after a ZIP-215 call the list holds over-long vectors only (keys on the curve), and the verdict is the
// cofactored one (ed_verify_zip215_reference_order); same protocol (slow_report, the completion word of a call of one)
__global__ void __launch_bounds__(ED_BLOCK, 2) k_ed25519_verify_slow_zip215(FastScratch fs, int* verdict, const void* sig, const void* pk,
                                                                            Msgs msgs, const u32* __restrict__ g_tbl, DoneWord done)
{
    const u32 count = *fs.slow_count;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *fs.slow_report = count;
        if (count == 0) signal_done(done);
    }
    if ((size_t)blockIdx.x * ED_BLOCK >= count) return;
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[PA_WORDS * 256];
    lds_stage_words(lds_tbl, g_tbl + REF_TBL_OFFSET, REF_TBL_WORDS);
    const size_t k = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (k >= count) return;
    const size_t i = fs.slow_list[k];
    u32 pkw[8], Rw[8], Sw[8];
    load32(pkw, pk, i);
    load32(Rw, sig, 2 * i);
    load32(Sw, sig, 2 * i + 1);
    verdict[i] = ed_verify_zip215_reference_order(pkw, Rw, Sw, msgs.ptr(i), msgs.len(i), fs.tables + i * FAST_TABLE_WORDS, lds_tbl);
    if (k == 0) signal_done(done);
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

// ---- ed25519_ClassifyKey_*, ed25519_PublicKey_to_X25519_*, ed25519_PrivateKey_to_X25519_* (ed_keys.cuh) -----------------------------------
// One lane per key at every size: the lane's work is the walk [L]A, 252 doublings and 45 additions on one extended point and one
// affine one, so the kernels take the registers two waves per SIMD leave them.
constexpr int EK_BLOCK = 256;
__global__ void __launch_bounds__(EK_BLOCK, 2) k_ed25519_key_classify(u32* flags, const void* pk, size_t n)
{
    const size_t i = (size_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    load32(w, pk, i);
    fe X, Y;
    flags[i] = ed_key_classify(X, Y, w);
}

// 1 + y, 1 - y and the ok word (all-ones / zero) to the scratch, ok[i] = 1 / 0 to the caller; k_batch_invert<FinishKeyX25519> writes xpk
__global__ void __launch_bounds__(EK_BLOCK, 2) k_ed25519_key_to_x25519(ProjScratch scr, int* ok, const void* pk, size_t n)
{
    const size_t i = (size_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    load32(w, pk, i);
    fe num, den;
    const u32 accept = ed_key_to_x25519_lane(num, den, w);
    soa_store_fe(scr.a, n, i, num);
    soa_store_fe(scr.z, n, i, den);
    scr.b[i] = accept;
    ok[i] = accept ? 1 : 0;
}

__global__ void __launch_bounds__(EK_BLOCK) k_ed25519_private_to_x25519(void* xsk, const void* priv, size_t n)
{
    const size_t i = (size_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    if (i >= n) return;
    ed_key_private_to_x25519(xsk, priv, i);
}

namespace {

// scratch of one verification pass: per-lane tables (the larger of the two paths' formats: they never live at the same
// time for one element), projective results of the reference-order path (the fast path keeps its decoded points there),
// the fast path's scalars, flags and slow list
constexpr size_t VERIFY_TABLE_WORDS = FAST_TABLE_WORDS > QTABLE_LIMB_WORDS ? FAST_TABLE_WORDS : QTABLE_LIMB_WORDS;
static_assert(FAST_TABLE_WORDS % 32 == 0 && VERIFY_TABLE_WORDS % 32 == 0, "per-lane tables must keep their rows 128-byte aligned");
inline size_t verify_scalar_words(size_t n) { return round_up(SIGMA_WORDS * n, 4) + 2 * round_up(5 * n, 4) + 5 * round_up(n, 4) + 4; }
inline size_t verify_scratch_bytes(size_t n)
{
    return (n * VERIFY_TABLE_WORDS + proj_words(n) + verify_scalar_words(n)) * sizeof(u32);
}

// fast = true: the lattice path (verify_fast.cuh) decides every element whose key is on the curve and whose short vector
// fits; the reference's order runs for the others in a kernel of its own behind the walk.  fast = false: reference order for everything,
// and Fin decides what leaves it: the verdict, or enc(T) for the test hook.
// what the calling thread's last fast-path verification left behind for c25519_amd_verify_last_slow_elements
struct LastVerify { const u32* count = nullptr; hipStream_t stream = nullptr; int device = -1; unsigned long generation = 0; };
thread_local LastVerify tl_last_verify;


// what the calling thread's last ed25519_Verify_Check_* call on this device left behind for c25519_amd_verify_check_last_wide:
// where its "the two wide combs decide this batch" word lives (null: the call never asked)
struct LastCheck { const u32* wide_ok = nullptr; hipStream_t stream = nullptr; int device = -1; unsigned long generation = 0; bool ran = false; };
thread_local LastCheck tl_last_check;

// rules (fast only): engine_common.cuh: VerifyRules
template <typename MakeFin>
int verify_run(const void* sig, const void* pk, Msgs msgs, size_t n, hipStream_t stream, int* verdict, bool fast, MakeFin make_fin,
               VerifyRules rules = RULES_PLAIN, bool last_in_call = true)
{
    const bool strict = rules == RULES_STRICT, zip215 = rules == RULES_ZIP215;
    const u32* tbl = nullptr;
    C25519_RC(base_tables(&tbl, nullptr));
    void* w = nullptr;
    c25519_host::WorkLease lease;
    C25519_RC(lease.acquire(&w, verify_scratch_bytes(n), stream));
    u32* tables = (u32*)w;                                  // first in the slab (hipMalloc: 256-byte aligned): packed rows are
    const ProjScratch scr = carve_proj(tables + n * VERIFY_TABLE_WORDS, n);   // whole 128-byte lines
    const unsigned grid = grid_for(n, ED_BLOCK);
    if (fast) {
        unsigned* report = nullptr;
        C25519_RC(tls().report_word_for(&report, stream));
        FastScratch fs;
        fs.tables = tables;
        fs.sigma = tables + n * VERIFY_TABLE_WORDS + proj_words(n);
        fs.rho = fs.sigma + round_up(SIGMA_WORDS * n, 4);
        fs.tau = fs.rho + round_up(5 * n, 4);
        fs.flags = fs.tau + round_up(5 * n, 4);
        fs.slow_list = fs.flags + round_up(n, 4);
        fs.order = fs.slow_list + round_up(n, 4);
        fs.slow_count = fs.order + round_up(n, 4);
        fs.pflags = fs.slow_count + 4;
        fs.slow_report = report;
        {   // test knob: a lower cap sends ordinary signatures down the over-long-vector branch (slow list, reference order)
            const long cap = c25519_host::tunable_or(c25519_host::T_VERIFY_LAT_CAP_BITS, LAT_CAP_BITS);
            fs.lat_cap_bits = cap >= 100 && cap < LAT_CAP_BITS ? (int)cap : LAT_CAP_BITS;
        }
        if (!verify_quad_for(n) && verify_coop_for(n)) {   // a few elements: one launch, three waves per element
            C25519_TRY(hipMemsetAsync(fs.slow_count, 0, 3 * sizeof(u32), stream));
            note_shape(SHAPE_PER_GROUP, 192);
            (zip215 ? k_ed25519_verify_one_per_group_zip215 : strict ? k_ed25519_verify_one_per_group_strict : k_ed25519_verify_one_per_group)<<<(unsigned)n, 192, 0, stream>>>(
                fs, verdict, sig, pk, msgs, n, tbl);
            C25519_TRY(hipGetLastError());
        } else if (verify_quad_for(n)) {                   // four lanes per element walk; scalars and points side by side in one launch
            const unsigned sb = grid_for(n, FS_BLOCK);
            note_shape(SHAPE_QUAD, QW_BLOCK);
            (zip215 ? k_ed25519_verify_quad_prep_zip215 : strict ? k_ed25519_verify_quad_prep_strict : k_ed25519_verify_quad_prep)<<<sb + grid_for(2 * n, ED_BLOCK), ED_BLOCK, 0, stream>>>(
                fs, sig, pk, msgs, n, sb);
            C25519_TRY(hipGetLastError());
            (zip215 ? k_ed25519_verify_quad_walk_zip215 : strict ? k_ed25519_verify_quad_walk_strict : k_ed25519_verify_quad_walk)<<<grid_for(n, QW_BLOCK / 4), QW_BLOCK, 0, stream>>>(
                fs, verdict, n, tbl);
            C25519_TRY(hipGetLastError());
        } else {
            note_shape(SHAPE_LANE, WALK_BLOCK);               // (no inversion on the lattice path: the walk decides)
            (zip215 ? k_ed25519_verify_fast_scalars_zip215 : strict ? k_ed25519_verify_fast_scalars_strict : k_ed25519_verify_fast_scalars)<<<grid_for(n, FS_BLOCK), FS_BLOCK, 0, stream>>>(
                fs, sig, pk, msgs, n);
            C25519_TRY(hipGetLastError());
            if (zip215)
                k_ed25519_verify_fast_points_zip215<<<grid_for(2 * n, ED_BLOCK), ED_BLOCK, 0, stream>>>(fs, sig, pk, n, verdict);
            else if (strict)
                k_ed25519_verify_fast_points_strict<<<grid_for(2 * n, ED_BLOCK), ED_BLOCK, 0, stream>>>(fs, sig, pk, n, verdict);
            else
                k_ed25519_verify_fast_points<<<grid_for(2 * n, ED_BLOCK), ED_BLOCK, 0, stream>>>(fs, sig, pk, n);
            C25519_TRY(hipGetLastError());
            // (strict, ZIP-215: rejected = listed; ZIP-215: the scalars came multiplied by 8, so the neutral test is the cofactored one)
            k_ed25519_verify_fast_walk<<<grid_for(n, WALK_BLOCK), WALK_BLOCK, 0, stream>>>(fs, verdict, n, tbl);
            C25519_TRY(hipGetLastError());
        }
        (zip215 ? k_ed25519_verify_slow_zip215 : k_ed25519_verify_slow)<<<grid, ED_BLOCK, 0, stream>>>(fs, verdict, sig, pk, msgs, tbl,
                                                                                                     last_in_call ? take_done_word(n) : DoneWord{ nullptr, 0 });
        C25519_TRY(hipGetLastError());
        tl_last_verify.count = report; tl_last_verify.stream = stream;
        tl_last_verify.generation = tls().generation;       // the report word and the stream die with the thread's slabs
        (void)hipGetDevice(&tl_last_verify.device);
        return lease.release();
    }
    tl_last_verify = LastVerify();
    note_shape(SHAPE_LANE_INVERT, ED_BLOCK);
    k_ed25519_verify_init<QTableLimbs><<<grid, ED_BLOCK, 0, stream>>>(pk, n, tables, VERIFY_TABLE_WORDS);
    C25519_TRY(hipGetLastError());
    k_ed25519_verify_check<QTableLimbs><<<grid, ED_BLOCK, 0, stream>>>(scr, sig, pk, msgs, n, tbl, tables, VERIFY_TABLE_WORDS);
    C25519_TRY(hipGetLastError());
    C25519_RC(launch_invert(scr, n, make_fin(scr), stream));
    return lease.release();
}

}  // namespace

int c25519_engine::verify_dev(void* verdict, const void* sig, const void* pk, Msgs msgs, size_t n, hipStream_t stream, VerifyRules rules,
                              bool last_in_call)
{
    // tunable VERIFY_REFERENCE_ORDER = 1: every element through the reference-order kernels -- Verify_Init's 4-fold table per
    // key, then the 4-fold + 8-fold walk of ed25519_verify.c:243-280: BASELINE.json configs[3] as worded (A/B and test knob).
    // The strict and the ZIP-215 calls always take the lattice path: their rules live in its kernels.
    const bool fast = rules != RULES_PLAIN || c25519_host::tunable_or(c25519_host::T_VERIFY_REFERENCE_ORDER, 0) == 0;
    if (int rc = check_dev_args(n, { verdict, sig, pk })) return rc;
    if (n == 0) return 0;
    return verify_run(sig, pk, msgs, n, stream, (int*)verdict, fast,
                      [&](const ProjScratch& scr) { return FinishVerify{ scr.a, scr.b, sig, (int*)verdict, n, nullptr }; }, rules, last_in_call);
}

extern "C" {

size_t ed25519_VerifySignature_scratch_bytes(size_t n) { return verify_scratch_bytes(n); }

// test hook: enc(T) instead of the verdict (what Verify_Check compares with enc(R)); device pointers
int c25519_amd_verify_point_dev(void* out, const void* sig, const void* pk, const void* msg, size_t msg_size, size_t n,
                                void* stream)
{
    C25519_API_CALL();
    if (!out || !sig || !pk || (!msg && msg_size)) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { out, sig, pk })) return rc;
    if (n == 0) return 0;
    return verify_run(sig, pk, fixed_msgs(msg, msg_size), n, (hipStream_t)stream, nullptr, false,
                      [&](const ProjScratch& scr) { return FinishPack{ scr.a, scr.b, out, n, 1, 0, nullptr, 0, 0 }; });
}

// how many elements of the calling thread's last ed25519_VerifySignature_* call on this device went through the
// reference-order kernel instead of the lattice path (-1: no fast-path verification to report).  Synchronises.
long c25519_amd_verify_last_slow_elements(void)
{
    C25519_API_CALL_OR(-1);
    const LastVerify& lv = tl_last_verify;
    int dev = -1;
    if (!lv.count || hipGetDevice(&dev) != hipSuccess || dev != lv.device) return -1;
    if (lv.generation != tls().generation) return -1;       // c25519_amd_thread_release() / a device switch freed what lv points at
    if (hipStreamSynchronize(lv.stream) != hipSuccess) return -1;
    u32 c = 0;
    if (hipMemcpy(&c, lv.count, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (long)c;
}

int ed25519_VerifySignature_dev(void* verdict, const void* sig, const void* pk, const void* msg, size_t msg_size,
                                size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !sig || !pk || (!msg && msg_size)) return bad_arg("null pointer");
    return verify_dev(verdict, sig, pk, fixed_msgs(msg, msg_size), n, (hipStream_t)stream, RULES_PLAIN);
}

int ed25519_VerifySignature_ragged_dev(void* verdict, const void* sig, const void* pk, const void* msgs,
                                       const uint64_t* offsets, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !sig || !pk || !offsets) return bad_arg("null pointer");
    return verify_dev(verdict, sig, pk, ragged_msgs(msgs, offsets), n, (hipStream_t)stream, RULES_PLAIN);
}

int ed25519_VerifySignature_strict_dev(void* verdict, const void* sig, const void* pk, const void* msg, size_t msg_size,
                                       size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !sig || !pk || (!msg && msg_size)) return bad_arg("null pointer");
    return verify_dev(verdict, sig, pk, fixed_msgs(msg, msg_size), n, (hipStream_t)stream, RULES_STRICT);
}

int ed25519_VerifySignature_strict_ragged_dev(void* verdict, const void* sig, const void* pk, const void* msgs,
                                              const uint64_t* offsets, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !sig || !pk || !offsets) return bad_arg("null pointer");
    return verify_dev(verdict, sig, pk, ragged_msgs(msgs, offsets), n, (hipStream_t)stream, RULES_STRICT);
}

// the ZIP-215 verdict (include/curve25519_amd.h): same arguments, dispatch and tunables as ed25519_VerifySignature_dev
int ed25519_VerifySignature_zip215_dev(void* verdict, const void* sig, const void* pk, const void* msg, size_t msg_size,
                                       size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !sig || !pk || (!msg && msg_size)) return bad_arg("null pointer");
    return verify_dev(verdict, sig, pk, fixed_msgs(msg, msg_size), n, (hipStream_t)stream, RULES_ZIP215);
}

int ed25519_VerifySignature_zip215_ragged_dev(void* verdict, const void* sig, const void* pk, const void* msgs,
                                              const uint64_t* offsets, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!verdict || !sig || !pk || !offsets) return bad_arg("null pointer");
    return verify_dev(verdict, sig, pk, ragged_msgs(msgs, offsets), n, (hipStream_t)stream, RULES_ZIP215);
}

// ---- ed25519_Verify_Check_zip215_*: host side (the kernels: above, behind the lattice path's ZIP-215 twins) --------------------------------
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
    const int K = inversion_group(std::min(inversion_k(n), 12));
    const size_t m = (n + K - 1) / K;
    const unsigned grid = grid_for(m, INV_BLOCK);
    switch (K) {
        case 12: k_batch_invert<FinishVerifyZip215, 12><<<grid, INV_BLOCK, 0, stream>>>(scr.prefix, nullptr, n, m, fin); break;
        case 8:  k_batch_invert<FinishVerifyZip215, 8><<<grid, INV_BLOCK, 0, stream>>>(scr.prefix, nullptr, n, m, fin); break;
        case 4:  k_batch_invert<FinishVerifyZip215, 4><<<grid, INV_BLOCK, 0, stream>>>(scr.prefix, nullptr, n, m, fin); break;
        case 2:  k_batch_invert<FinishVerifyZip215, 2><<<grid, INV_BLOCK, 0, stream>>>(scr.prefix, nullptr, n, m, fin); break;
        default: k_batch_invert<FinishVerifyZip215, 1><<<grid, INV_BLOCK, 0, stream>>>(scr.prefix, nullptr, n, m, fin); break;
    }
    C25519_TRY(hipGetLastError());
    return 0;
}

// the keys gathered behind the per-element call's scratch, then that call (ctx_index null: one context)
static int zip215_check_gathered(int* verdict, const void* ctxs, size_t n_ctx, const void* ctx_index, const void* sig, Msgs msgs, size_t n,
                                 hipStream_t stream)
{
    const size_t inner = round_up(ed25519_VerifySignature_scratch_bytes(n), 256);
    void* w = nullptr;
    c25519_host::WorkLease lease;
    C25519_RC(lease.acquire(&w, inner + n * 32, stream));
    void* pk = (char*)w + inner;
    k_ed25519_verify_coset_key_gather<<<grid_for(n, ZC_BLOCK), ZC_BLOCK, 0, stream>>>(pk, (const u32*)ctxs, n_ctx, (const u32*)ctx_index, n);
    C25519_TRY(hipGetLastError());
    C25519_RC(verify_dev(verdict, sig, pk, msgs, n, stream, RULES_ZIP215, /* last_in_call = */ false));
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
    tl_last_check = LastCheck();
    tl_last_check.ran = true;
    if (!zip215 && !try_wide && small) {                    // a few pairs: one per wave, the reference's order
        k_ed25519_verify_check_coop<<<(unsigned)n, 64, 0, stream>>>((int*)verdict, sig, (const u32*)ctx, msgs, n, tbl, take_done_word(n));
        C25519_TRY(hipGetLastError());
        return 0;
    }
    void* w = nullptr;
    c25519_host::WorkLease lease;
    C25519_RC(lease.acquire(&w, (proj_words(n) + 4) * sizeof(u32), stream));
    const ProjScratch scr = carve_proj((u32*)w, n);
    u32* wide_ok = nullptr;
    bool quads = false;
    c25519_host::KeepLease keep_lease;                      // records the kept buffer's event however this call leaves
    if (try_wide) {
        const u32* wide_base = nullptr;
        C25519_RC(wide_tables(&wide_base));
        // the key's comb and the context it was built for live in a buffer of the calling thread that outlives the call
        // (ThreadState::keep): the next call with the same context bytes finds them there.  The verdict on THIS call's context
        // (wide_ok) is the call's own: a word of its work scratch.
        void* keep = nullptr;
        bool fresh = false;
        constexpr size_t KEEP_WORDS = WB_TBL_WORDS + 16 * 32 + KEEP_CTX_WORDS + 1 + 3;
        C25519_RC(keep_lease.acquire(&keep, KEEP_WORDS * sizeof(u32), stream, &fresh));
        u32* wide_key = (u32*)keep;
        u32* check_rows = wide_key + WB_TBL_WORDS;
        u32* remembered = check_rows + 16 * 32;
        wide_ok = (u32*)w + proj_words(n);                  // (16-byte aligned: proj_words is a multiple of 4)
        tl_last_check.wide_ok = wide_ok; tl_last_check.stream = stream; tl_last_check.generation = tls().generation;
        (void)hipGetDevice(&tl_last_check.device);
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
    if (zip215) {                                           // rule 2 for the one context: word 1 behind the projective part
        u32* key_ok = (u32*)w + proj_words(n) + 1;
        C25519_RC(launch_coset_finish(scr, n, (const u32*)ctx, 1, nullptr, key_ok, sig, (int*)verdict, stream));
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
    const size_t row_words = C25519_INDEXED_REPACK ? n_ctx * QTABLE_CANON_WORDS : 0;
    void* w = nullptr;
    c25519_host::WorkLease lease;
    C25519_RC(lease.acquire(&w, (row_words + proj_words(n) + (zip215 ? round_up(n_ctx, 4) : 0)) * sizeof(u32), stream));
    u32* rows = (u32*)w;                                    // first in the slab (hipMalloc: 256-byte aligned): whole 128-byte rows
    const ProjScratch scr = carve_proj(rows + row_words, n);
#if C25519_INDEXED_REPACK
    k_ed25519_verify_ctx_repack<<<grid_for(n_ctx * (QTABLE_CANON_WORDS / 4), 256), 256, 0, stream>>>((uint4*)rows, (const u32*)ctxs, n_ctx);
    C25519_TRY(hipGetLastError());
#endif
    k_ed25519_verify_check_indexed<<<grid_for(n, ED_BLOCK), ED_BLOCK, 0, stream>>>(scr, sig, (const u32*)ctxs, n_ctx, (const u32*)ctx_index,
                                                                                  msgs, n, tbl, rows);
    C25519_TRY(hipGetLastError());
    if (zip215)                                             // rule 2 per context: n_ctx words behind the projective part
        C25519_RC(launch_coset_finish(scr, n, (const u32*)ctxs, n_ctx, (const u32*)ctx_index, rows + row_words + proj_words(n), sig,
                                      (int*)verdict, stream));
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
        tl_last_check = LastCheck();
        tl_last_check.ran = true;
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
    const LastCheck& lc = tl_last_check;
    if (!lc.ran) return -1;
    if (!lc.wide_ok) return 0;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != lc.device || lc.generation != tls().generation) return -1;
    if (hipStreamSynchronize(lc.stream) != hipSuccess) return -1;
    u32 v = 0;
    if (hipMemcpy(&v, lc.wide_ok, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return v ? 1 : 0;
}

// ---- key classification and conversion (the kernels: above, behind the coset kernels; the rules: include/curve25519_amd.h) ----------------
// One lane per key at every n; c25519_amd_last_shape is not written.

int ed25519_ClassifyKey_dev(void* flags, const void* pk, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!flags || !pk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { flags, pk })) return rc;
    if (n == 0) return 0;
    k_ed25519_key_classify<<<grid_for(n, EK_BLOCK), EK_BLOCK, 0, (hipStream_t)stream>>>((u32*)flags, pk, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ed25519_PublicKey_to_X25519_dev(void* xpk, void* ok, const void* pk, size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!xpk || !ok || !pk) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { xpk, ok, pk })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    void* w = nullptr;
    c25519_host::WorkLease lease;
    C25519_RC(lease.acquire(&w, proj_words(n) * sizeof(u32), stream));
    const ProjScratch scr = carve_proj((u32*)w, n);           // a = 1 + y, z = 1 - y, b = the ok words (n of its 10 n)
    k_ed25519_key_to_x25519<<<grid_for(n, EK_BLOCK), EK_BLOCK, 0, stream>>>(scr, (int*)ok, pk, n);
    C25519_TRY(hipGetLastError());
    C25519_RC(launch_invert(scr, n, FinishKeyX25519{ scr.a, scr.b, xpk, n }, stream));
    return lease.release();
}

int ed25519_PrivateKey_to_X25519_dev(void* xsk, const void* priv, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!xsk || !priv) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { xsk, priv })) return rc;
    if (n == 0) return 0;
    k_ed25519_private_to_x25519<<<grid_for(n, EK_BLOCK), EK_BLOCK, 0, (hipStream_t)stream>>>(xsk, priv, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
