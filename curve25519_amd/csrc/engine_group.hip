// curve25519_amd/csrc/engine_group.hip -- ed25519_ScalarMult[_noclamp]_*, ed25519_ScalarMultBase[_noclamp]_*, ed25519_PointAdd_*,
// ed25519_PointSub_*: the group operations (the lane's work: ed_group.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "ed_group.cuh"

// One lane per element at every size.  The variable-base walk keeps its table in registers, 2 / 4 / 8 rows of 40 limbs beside the
// running point: two waves per SIMD at W = 2, the whole register file of a SIMD (accumulator registers included) at W = 3 and 4.
constexpr int EG_BLOCK = 256;
// the width that is fastest at 2^20 by more than the rounds' spread: 11.60 ms against 12.15 (W = 3) and 11.99 (W = 4), spread 0.07
// (tools/group_ops_rate.py, profiles/group_ops_rate.txt); in a latency-bound call (up to 2^16) W = 3 and 4 are ~9 % shorter
constexpr int SCALARMULT_WINDOW_DEFAULT = 2;

// X, Y, Z and the ok word (all-ones / zero) to the scratch, ok[i] = 1 / 0 to the caller; k_batch_invert<FinishGroupPoint> writes q
template <int W>
__global__ void __launch_bounds__(EG_BLOCK, W == 2 ? 2 : 1) k_ed25519_group_scalarmult(ProjScratch scr, u32* okw, int* ok, const void* scalar,
                                                                                      const void* point, u32 clamp, size_t n)
{
    const size_t i = (size_t)blockIdx.x * EG_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 sw[8], pw[8];
    load32(sw, scalar, i);
    load32(pw, point, i);
    ge_ext S;
    const u32 accept = ed_group_scalarmult_lane<W>(S, sw, pw, clamp);
    store_proj(scr, n, i, S);
    okw[i] = accept;
    ok[i] = accept ? 1 : 0;
}

// [e]B over the wide comb, whatever the call's size; k_batch_invert<FinishPack> writes q
__global__ void __launch_bounds__(WB_BLOCK, 4) k_ed25519_group_base(ProjScratch scr, const void* scalar, u32 clamp, size_t n,
                                                                    const u32* __restrict__ g_wide)
{
    __shared__ unsigned short cols[WB_COLS * WB_BLOCK];
    const size_t i = (size_t)blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 sw[8];
    load32(sw, scalar, i);
    ge_ext S;
    ed_group_base_lane(S, sw, clamp, g_wide, cols + threadIdx.x, WB_BLOCK);
    store_proj(scr, n, i, S);
}

// P + Q (negate = zero) or P - Q (all-ones)
__global__ void __launch_bounds__(EG_BLOCK, 2) k_ed25519_group_add(ProjScratch scr, u32* okw, int* ok, const void* p, const void* q, u32 negate,
                                                                   size_t n)
{
    const size_t i = (size_t)blockIdx.x * EG_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pw[8], qw[8];
    load32(pw, p, i);
    load32(qw, q, i);
    ge_ext S;
    const u32 accept = ed_group_add_lane(S, pw, qw, negate);
    store_proj(scr, n, i, S);
    okw[i] = accept;
    ok[i] = accept ? 1 : 0;
}

namespace {

// the scratch of a call: the projective part, then (a call with an ok word per element) n words
struct GroupScratch { ProjScratch scr; u32* okw; };
int lease_group(GroupScratch* g, c25519_host::WorkLease& lease, size_t n, bool ok_words, hipStream_t stream)
{
    return lease_scratch(g, lease, stream, [=](Carve& c) {
        GroupScratch s;
        s.scr = c.proj(n);
        s.okw = c.take4(ok_words ? n : 0);
        return s;
    });
}

// tunable SCALARMULT_WINDOW: 2, 3 or 4; anything else is the built-in choice
int scalarmult_window()
{
    const long v = c25519_host::tunable(c25519_host::T_SCALARMULT_WINDOW);
    return v >= 2 && v <= 4 ? (int)v : SCALARMULT_WINDOW_DEFAULT;
}

int scalarmult_dev(void* q, void* ok, const void* scalar, const void* point, size_t n, void* stream_, bool clamp)
{
    C25519_API_CALL();
    if (!q || !ok || !scalar || !point) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { q, ok, scalar, point })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    GroupScratch g;
    c25519_host::WorkLease lease;
    C25519_RC(lease_group(&g, lease, n, true, stream));
    const unsigned grid = grid_for(n, EG_BLOCK);
    const u32 cm = clamp ? 0xffffffffu : 0u;
    switch (scalarmult_window()) {
        case 4:  k_ed25519_group_scalarmult<4><<<grid, EG_BLOCK, 0, stream>>>(g.scr, g.okw, (int*)ok, scalar, point, cm, n); break;
        case 3:  k_ed25519_group_scalarmult<3><<<grid, EG_BLOCK, 0, stream>>>(g.scr, g.okw, (int*)ok, scalar, point, cm, n); break;
        default: k_ed25519_group_scalarmult<2><<<grid, EG_BLOCK, 0, stream>>>(g.scr, g.okw, (int*)ok, scalar, point, cm, n); break;
    }
    C25519_TRY(hipGetLastError());
    C25519_RC(launch_invert(g.scr, n, FinishGroupPoint{ g.scr.a, g.scr.b, g.okw, q, n }, stream));
    return lease.release();
}

int scalarmult_base_dev(void* q, const void* scalar, size_t n, void* stream_, bool clamp)
{
    C25519_API_CALL();
    if (!q || !scalar) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { q, scalar })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    GroupScratch g;
    c25519_host::WorkLease lease;
    C25519_RC(lease_group(&g, lease, n, false, stream));
    k_ed25519_group_base<<<grid_for(n, WB_BLOCK), WB_BLOCK, 0, stream>>>(g.scr, scalar, clamp ? 0xffffffffu : 0u, n, wide);
    C25519_TRY(hipGetLastError());
    C25519_RC(launch_invert(g.scr, n, FinishPack{ g.scr.a, g.scr.b, q, n, 1, 0, nullptr, 0, 0 }, stream));
    return lease.release();
}

int point_add_dev(void* r, void* ok, const void* p, const void* q, size_t n, void* stream_, bool sub)
{
    C25519_API_CALL();
    if (!r || !ok || !p || !q) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { r, ok, p, q })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    GroupScratch g;
    c25519_host::WorkLease lease;
    C25519_RC(lease_group(&g, lease, n, true, stream));
    k_ed25519_group_add<<<grid_for(n, EG_BLOCK), EG_BLOCK, 0, stream>>>(g.scr, g.okw, (int*)ok, p, q, sub ? 0xffffffffu : 0u, n);
    C25519_TRY(hipGetLastError());
    C25519_RC(launch_invert(g.scr, n, FinishGroupPoint{ g.scr.a, g.scr.b, g.okw, r, n }, stream));
    return lease.release();
}

}  // namespace

extern "C" {

// (the rules: include/curve25519_amd.h)  One lane per element at every n; c25519_amd_last_shape is not written.

int ed25519_ScalarMult_dev(void* q, void* ok, const void* scalar, const void* point, size_t n, void* stream)
{
    return scalarmult_dev(q, ok, scalar, point, n, stream, true);
}

int ed25519_ScalarMult_noclamp_dev(void* q, void* ok, const void* scalar, const void* point, size_t n, void* stream)
{
    return scalarmult_dev(q, ok, scalar, point, n, stream, false);
}

int ed25519_ScalarMultBase_dev(void* q, const void* scalar, size_t n, void* stream) { return scalarmult_base_dev(q, scalar, n, stream, true); }

int ed25519_ScalarMultBase_noclamp_dev(void* q, const void* scalar, size_t n, void* stream)
{
    return scalarmult_base_dev(q, scalar, n, stream, false);
}

int ed25519_PointAdd_dev(void* r, void* ok, const void* p, const void* q, size_t n, void* stream) { return point_add_dev(r, ok, p, q, n, stream, false); }

int ed25519_PointSub_dev(void* r, void* ok, const void* p, const void* q, size_t n, void* stream) { return point_add_dev(r, ok, p, q, n, stream, true); }

}  // extern "C"
