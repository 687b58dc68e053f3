// curve25519_amd/csrc/engine_ristretto.hip -- ristretto255_IsValidPoint_*, ristretto255_FromHash_*, ristretto255_ScalarMult_*,
// ristretto255_ScalarMultBase_*, ristretto255_PointAdd_*, ristretto255_PointSub_*: the prime-order group of RFC 9496 (the lane's
// work: ristretto255.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "ristretto255.cuh"

// One lane per element at every size, ONE kernel per call: the encoding's inverse square root is the lane's own (ristretto255.cuh
// says why it is not shared), so no call leases scratch or launches k_batch_invert.  The register budgets are the group kernels':
// two waves per SIMD for the walk at W = 2 (decode runs before the table exists, encode after it is dead), the whole register file
// of a SIMD at W = 3 and 4.  The comb kernel runs two waves per SIMD where the group calls' runs four: the encoding holds the point,
// u1, u2 and the chain's intermediates, 180 registers.
constexpr int RIST_BLOCK = 256;
// the width that is fastest at 2^20 by more than the rounds' spread, and the group calls' built-in width too: 12.16 ms against 12.71
// (W = 3) and 12.99 (W = 4), spread 0.02 (tools/ristretto_rate.py, profiles/ristretto_rate.txt); up to 2^16 W = 3 is ~10 % shorter
constexpr int RIST_WINDOW_DEFAULT = 2;

__global__ void __launch_bounds__(RIST_BLOCK, 2) k_ristretto255_is_valid(int* ok, const void* point, size_t n)
{
    const size_t i = (size_t)blockIdx.x * RIST_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pw[8];
    load32(pw, point, i);
    fe X, Y;
    ok[i] = (int)(rist_decode(X, Y, pw, 0u) & 1u);
}

// hash: n x 64 bytes, rows 2 i and 2 i + 1 of 32
__global__ void __launch_bounds__(RIST_BLOCK, 2) k_ristretto255_from_hash(void* p, const void* hash, size_t n)
{
    const size_t i = (size_t)blockIdx.x * RIST_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 lo[8], hi[8], out[8];
    load32(lo, hash, 2 * i);
    load32(hi, hash, 2 * i + 1);
    rist_from_hash_lane(out, lo, hi);
    store32(p, i, out);
}

// decode -> ed_group_walk<W> -> encode
template <int W>
__global__ void __launch_bounds__(RIST_BLOCK, W == 2 ? 2 : 1) k_ristretto255_scalarmult(void* q, int* ok, const void* scalar, const void* point, size_t n)
{
    const size_t i = (size_t)blockIdx.x * RIST_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 sw[8], pw[8], out[8];
    load32(sw, scalar, i);
    load32(pw, point, i);
    const u32 accept = rist_scalarmult_lane<W>(out, sw, pw);
    store32(q, i, out);
    ok[i] = (int)(accept & 1u);
}

// [e]B over the wide comb -> encode
__global__ void __launch_bounds__(WB_BLOCK, 2) k_ristretto255_base(void* q, const void* scalar, size_t n, const u32* __restrict__ g_wide)
{
    __shared__ unsigned short cols[WB_COLS * WB_BLOCK];
    const size_t i = (size_t)blockIdx.x * WB_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 sw[8], out[8];
    load32(sw, scalar, i);
    rist_base_lane(out, sw, g_wide, cols + threadIdx.x, WB_BLOCK);
    store32(q, i, out);
}

// P + Q (negate = zero) or P - Q (all-ones)
__global__ void __launch_bounds__(RIST_BLOCK, 2) k_ristretto255_add(void* r, int* ok, const void* p, const void* q, u32 negate, size_t n)
{
    const size_t i = (size_t)blockIdx.x * RIST_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pw[8], qw[8], out[8];
    load32(pw, p, i);
    load32(qw, q, i);
    const u32 accept = rist_add_lane(out, pw, qw, negate);
    store32(r, i, out);
    ok[i] = (int)(accept & 1u);
}

namespace {

// tunable SCALARMULT_WINDOW, as the group calls read it: 2, 3 or 4; anything else is the built-in choice
int rist_window()
{
    const long v = c25519_host::tunable(c25519_host::T_SCALARMULT_WINDOW);
    return v >= 2 && v <= 4 ? (int)v : RIST_WINDOW_DEFAULT;
}

int rist_point_add_dev(void* r, void* ok, const void* p, const void* q, size_t n, void* stream_, bool sub)
{
    C25519_API_CALL();
    if (!r || !ok || !p || !q) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { r, ok, p, q })) return rc;
    if (n == 0) return 0;
    k_ristretto255_add<<<grid_for(n, RIST_BLOCK), RIST_BLOCK, 0, (hipStream_t)stream_>>>(r, (int*)ok, p, q, sub ? 0xffffffffu : 0u, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

// (the rules: include/curve25519_amd.h)  One lane per element at every n; c25519_amd_last_shape is not written.

int ristretto255_IsValidPoint_dev(void* ok, const void* point, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!ok || !point) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { ok, point })) return rc;
    if (n == 0) return 0;
    k_ristretto255_is_valid<<<grid_for(n, RIST_BLOCK), RIST_BLOCK, 0, (hipStream_t)stream>>>((int*)ok, point, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ristretto255_FromHash_dev(void* p, const void* hash, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!p || !hash) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { p, hash })) return rc;
    if (n == 0) return 0;
    k_ristretto255_from_hash<<<grid_for(n, RIST_BLOCK), RIST_BLOCK, 0, (hipStream_t)stream>>>(p, hash, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ristretto255_ScalarMult_dev(void* q, void* ok, const void* scalar, const void* point, size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!q || !ok || !scalar || !point) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { q, ok, scalar, point })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned grid = grid_for(n, RIST_BLOCK);
    switch (rist_window()) {
        case 4:  k_ristretto255_scalarmult<4><<<grid, RIST_BLOCK, 0, stream>>>(q, (int*)ok, scalar, point, n); break;
        case 3:  k_ristretto255_scalarmult<3><<<grid, RIST_BLOCK, 0, stream>>>(q, (int*)ok, scalar, point, n); break;
        default: k_ristretto255_scalarmult<2><<<grid, RIST_BLOCK, 0, stream>>>(q, (int*)ok, scalar, point, n); break;
    }
    C25519_TRY(hipGetLastError());
    return 0;
}

int ristretto255_ScalarMultBase_dev(void* q, const void* scalar, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!q || !scalar) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { q, scalar })) return rc;
    if (n == 0) return 0;
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    k_ristretto255_base<<<grid_for(n, WB_BLOCK), WB_BLOCK, 0, (hipStream_t)stream>>>(q, scalar, n, wide);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ristretto255_PointAdd_dev(void* r, void* ok, const void* p, const void* q, size_t n, void* stream)
{
    return rist_point_add_dev(r, ok, p, q, n, stream, false);
}

int ristretto255_PointSub_dev(void* r, void* ok, const void* p, const void* q, size_t n, void* stream)
{
    return rist_point_add_dev(r, ok, p, q, n, stream, true);
}

}  // extern "C"
