// curve25519_amd/csrc/engine_verify.hip -- Ed25519 verification per element (ed25519_VerifySignature_*): the lattice path (scalars, points,
// walk; on quads; one launch of three waves) with its strict and ZIP-215 twins, and the reference order -- kernels and *_dev entry points.
// Verification against Verify_Init contexts is engine_verify_ctx.hip, which comes here through verify_dev and
// ed25519_VerifySignature_scratch_bytes only: what lands there or in engine_keys.hip does not reach this unit's kernels.
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "verify_check.cuh"

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

namespace {

// scratch of one verification pass: per-lane tables (the larger of the two paths' formats: they never live at the same
// time for one element), projective results of the reference-order path (the fast path keeps its decoded points there),
// the fast path's scalars, flags and slow list
constexpr size_t VERIFY_TABLE_WORDS = FAST_TABLE_WORDS > QTABLE_LIMB_WORDS ? FAST_TABLE_WORDS : QTABLE_LIMB_WORDS;
static_assert(FAST_TABLE_WORDS % 32 == 0 && VERIFY_TABLE_WORDS % 32 == 0, "per-lane tables must keep their rows 128-byte aligned");
constexpr size_t SLOW_COUNTERS = 3;          // FastScratch::slow_count: the count, then how many elements `order` holds from its front / its back
struct VerifyScratch { u32* tables; ProjScratch scr; FastScratch fs; };
inline VerifyScratch verify_layout(Carve& c, size_t n)
{
    VerifyScratch v;
    FastScratch& fs = v.fs;
    fs.tables = v.tables = c.take(n * VERIFY_TABLE_WORDS);  // first in the slab (hipMalloc: 256-byte aligned): packed rows are whole 128-byte lines
    v.scr = c.proj(n);
    fs.sigma = c.take4(SIGMA_WORDS * n);
    fs.rho = c.take4(5 * n);
    fs.tau = c.take4(5 * n);
    fs.flags = c.take4(n);
    fs.slow_list = c.take4(n);
    fs.order = c.take4(n);
    fs.slow_count = c.take4(SLOW_COUNTERS);
    fs.pflags = c.take(2 * round_up(n, 4));                 // key lanes, then R lanes: 2n words are indexed (R of e at n + e)
    fs.slow_report = nullptr;
    fs.lat_cap_bits = LAT_CAP_BITS;
    return v;
}

// what the calling thread's last fast-path verification left behind for c25519_amd_verify_last_slow_elements
thread_local c25519_host::LastCall tl_last_verify;

// fast = true: the lattice path (verify_fast.cuh) decides every element whose key is on the curve and whose short vector
// fits; the reference's order runs for the others in a kernel of its own behind the walk.  fast = false: reference order for everything,
// and Fin decides what leaves it: the verdict, or enc(T) for the test hook.
// rules (fast only): engine_common.cuh: VerifyRules
template <typename MakeFin>
int verify_run(const void* sig, const void* pk, Msgs msgs, size_t n, hipStream_t stream, int* verdict, bool fast, MakeFin make_fin,
               VerifyRules rules = RULES_PLAIN, bool last_in_call = true, u32* work = nullptr)
{
    const bool strict = rules == RULES_STRICT, zip215 = rules == RULES_ZIP215;
    const u32* tbl = nullptr;
    C25519_RC(base_tables(&tbl, nullptr));
    VerifyScratch v;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&v, lease, stream, [n](Carve& c) { return verify_layout(c, n); }, work));
    const ProjScratch& scr = v.scr;
    const unsigned grid = grid_for(n, ED_BLOCK);
    if (fast) {
        unsigned* report = nullptr;
        C25519_RC(tls().report_word_for(&report, c25519_host::REPORT_SLOW_ELEMENTS, stream));
        FastScratch& fs = v.fs;
        fs.slow_report = report;
        {   // test knob: a lower cap sends ordinary signatures down the over-long-vector branch (slow list, reference order)
            const long cap = c25519_host::tunable_or(c25519_host::T_VERIFY_LAT_CAP_BITS, LAT_CAP_BITS);
            fs.lat_cap_bits = cap >= 100 && cap < LAT_CAP_BITS ? (int)cap : LAT_CAP_BITS;
        }
        if (!verify_quad_for(n) && verify_coop_for(n)) {   // a few elements: one launch, three waves per element
            C25519_TRY(hipMemsetAsync(fs.slow_count, 0, SLOW_COUNTERS * sizeof(u32), stream));
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
        tl_last_verify.reports_in(report, stream);
        return lease.release();
    }
    tl_last_verify = c25519_host::LastCall();
    note_shape(SHAPE_LANE_INVERT, ED_BLOCK);
    k_ed25519_verify_init<QTableLimbs><<<grid, ED_BLOCK, 0, stream>>>(pk, n, v.tables, VERIFY_TABLE_WORDS);
    C25519_TRY(hipGetLastError());
    k_ed25519_verify_check<QTableLimbs><<<grid, ED_BLOCK, 0, stream>>>(scr, sig, pk, msgs, n, tbl, v.tables, VERIFY_TABLE_WORDS);
    C25519_TRY(hipGetLastError());
    C25519_RC(launch_invert(scr, n, make_fin(scr), stream));
    return lease.release();
}

}  // namespace

int c25519_engine::verify_dev(void* verdict, const void* sig, const void* pk, Msgs msgs, size_t n, hipStream_t stream, VerifyRules rules,
                              bool last_in_call, u32* work)
{
    // tunable VERIFY_REFERENCE_ORDER = 1: every element through the reference-order kernels -- Verify_Init's 4-fold table per
    // key, then the 4-fold + 8-fold walk of ed25519_verify.c:243-280: BASELINE.json configs[3] as worded (A/B and test knob).
    // The strict and the ZIP-215 calls always take the lattice path: their rules live in its kernels.
    const bool fast = rules != RULES_PLAIN || c25519_host::tunable_or(c25519_host::T_VERIFY_REFERENCE_ORDER, 0) == 0;
    if (int rc = check_dev_args(n, { verdict, sig, pk })) return rc;
    if (n == 0) return 0;
    return verify_run(sig, pk, msgs, n, stream, (int*)verdict, fast,
                      [&](const ProjScratch& scr) { return FinishVerify{ scr.a, scr.b, sig, (int*)verdict, n, nullptr }; }, rules, last_in_call, work);
}

extern "C" {

size_t ed25519_VerifySignature_scratch_bytes(size_t n) { return layout_bytes([n](Carve& c) { return verify_layout(c, n); }); }

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
    return tl_last_verify.read();
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

}  // extern "C"
