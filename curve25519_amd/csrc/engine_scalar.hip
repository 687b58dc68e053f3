// curve25519_amd/csrc/engine_scalar.hip -- ed25519_ScalarReduce_*, ed25519_ScalarAdd_*, ed25519_ScalarSub_*, ed25519_ScalarMul_*,
// ed25519_ScalarNegate_*, ed25519_ScalarComplement_*, ed25519_ScalarMulAdd_*, ed25519_ScalarInvert_*, ed25519_ScalarIsCanonical_*:
// arithmetic mod L, the base-point order (the lane's work: sc_invert.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "sc_invert.cuh"

// One lane per element (Invert: per group of K elements) at every size, ONE kernel per call, no scratch leased.  Two waves per SIMD
// leave a lane 256 registers: the inversion at K = 16 keeps nine prefix products in them and six in LDS (sc_invert.cuh says why).
constexpr int SC_BLOCK = 256;
// elements per inverting lane (tunable SC_INVERT_K: 1, 2, 4, 8 or 16; anything else is this choice): the smallest K that leaves every
// lane's group inside SC_INVERT_LANES_MAX lanes (256 CUs x 4 SIMDs x 64 lanes: one wave per SIMD), at most SC_INVERT_K_MAX.  That is
// what is fastest at each size by more than the rounds' spread (tools/scalar_rate.py, profiles/scalar_rate.txt; spreads of 0.000-0.003
// ms): K = 1 up to 2^16, 0.027-0.030 ms a call, one lane's inversion (K = 2: 0.031-0.033); K = 2 at 2^17, 0.035 ms against 0.043
// (K = 4) and 0.056 (K = 1); K = 4 at 2^18, 0.043 against 0.058-0.060; K = 8 at 2^19, 0.066 against 0.071, and at 2^20, 0.099 ms against
// 0.111 for K = 16.  While the lanes fit one wave per SIMD a call costs one lane's chain, which every doubling of K lengthens;
// beyond, the shared inversion pays, and K = 16's six prefix products in LDS cost more than its halved share of the inversion saves.
constexpr size_t SC_INVERT_LANES_MAX = 65536;
constexpr int SC_INVERT_K_MAX = 8;

// r = op(a, b, c) (sc_invert.cuh: ScOp)
__global__ void __launch_bounds__(SC_BLOCK, 2) k_sc25519_op(void* r, const void* a, const void* b, const void* c, int op, size_t n)
{
    const size_t i = (size_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= n) return;
    sc_op_lane(op, r, a, b, c, i);
}

__global__ void __launch_bounds__(SC_BLOCK, 2) k_sc25519_is_canonical(int* ok, const void* s, size_t n)
{
    const size_t i = (size_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    load32(w, s, i);
    ok[i] = (int)sc_is_canonical(w);
}

// lane i: elements i K .. i K + K - 1; m = ceil(n / K) lanes
template <int K>
__global__ void __launch_bounds__(SC_BLOCK, 2) k_sc25519_invert(void* recip, int* ok, const void* s, size_t n, size_t m)
{
    constexpr int PARK = sc_invert_parked<K>();
    __shared__ u32 park[PARK ? PARK * 8 * SC_BLOCK : 1];
    const size_t i = (size_t)blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= m) return;
    sc_invert_lane<K>(recip, ok, s, n, i, park + threadIdx.x, SC_BLOCK);
}

namespace {

int sc_invert_k(size_t n)
{
    const long v = c25519_host::tunable(c25519_host::T_SC_INVERT_K);
    if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) return (int)v;
    int k = 1;
    while (k < SC_INVERT_K_MAX && (n + k - 1) / k > SC_INVERT_LANES_MAX) k *= 2;
    return k;
}

// a, and b and c where the operation reads them, are checked; r may be any of them
int sc_op_dev(int op, void* r, const void* a, const void* b, const void* c, size_t n, void* stream)
{
    C25519_API_CALL();
    const bool two = op == SC_OP_ADD || op == SC_OP_SUB || op == SC_OP_MUL || op == SC_OP_MULADD, three = op == SC_OP_MULADD;
    if (!r || !a || (two && !b) || (three && !c)) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { r, a, two ? b : nullptr, three ? c : nullptr })) return rc;
    if (n == 0) return 0;
    k_sc25519_op<<<grid_for(n, SC_BLOCK), SC_BLOCK, 0, (hipStream_t)stream>>>(r, a, b, c, op, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

// (the rules: include/curve25519_amd.h)  c25519_amd_last_shape is not written.

int ed25519_ScalarReduce_dev(void* r, const void* s, size_t n, void* stream) { return sc_op_dev(SC_OP_REDUCE, r, s, nullptr, nullptr, n, stream); }
int ed25519_ScalarAdd_dev(void* z, const void* x, const void* y, size_t n, void* stream) { return sc_op_dev(SC_OP_ADD, z, x, y, nullptr, n, stream); }
int ed25519_ScalarSub_dev(void* z, const void* x, const void* y, size_t n, void* stream) { return sc_op_dev(SC_OP_SUB, z, x, y, nullptr, n, stream); }
int ed25519_ScalarMul_dev(void* z, const void* x, const void* y, size_t n, void* stream) { return sc_op_dev(SC_OP_MUL, z, x, y, nullptr, n, stream); }
int ed25519_ScalarNegate_dev(void* r, const void* s, size_t n, void* stream) { return sc_op_dev(SC_OP_NEGATE, r, s, nullptr, nullptr, n, stream); }
int ed25519_ScalarComplement_dev(void* r, const void* s, size_t n, void* stream) { return sc_op_dev(SC_OP_COMPLEMENT, r, s, nullptr, nullptr, n, stream); }
int ed25519_ScalarMulAdd_dev(void* r, const void* a, const void* b, const void* c, size_t n, void* stream)
{
    return sc_op_dev(SC_OP_MULADD, r, a, b, c, n, stream);
}

int ed25519_ScalarInvert_dev(void* recip, void* ok, const void* s, size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!recip || !ok || !s) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { recip, ok, s })) return rc;
    if (n == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const int K = sc_invert_k(n);
    const size_t m = (n + K - 1) / K;
    const unsigned grid = grid_for(m, SC_BLOCK);
    switch (K) {
        case 16: k_sc25519_invert<16><<<grid, SC_BLOCK, 0, stream>>>(recip, (int*)ok, s, n, m); break;
        case 8:  k_sc25519_invert<8><<<grid, SC_BLOCK, 0, stream>>>(recip, (int*)ok, s, n, m); break;
        case 4:  k_sc25519_invert<4><<<grid, SC_BLOCK, 0, stream>>>(recip, (int*)ok, s, n, m); break;
        case 2:  k_sc25519_invert<2><<<grid, SC_BLOCK, 0, stream>>>(recip, (int*)ok, s, n, m); break;
        default: k_sc25519_invert<1><<<grid, SC_BLOCK, 0, stream>>>(recip, (int*)ok, s, n, m); break;
    }
    C25519_TRY(hipGetLastError());
    return 0;
}

int ed25519_ScalarIsCanonical_dev(void* ok, const void* s, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!ok || !s) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { ok, s })) return rc;
    if (n == 0) return 0;
    k_sc25519_is_canonical<<<grid_for(n, SC_BLOCK), SC_BLOCK, 0, (hipStream_t)stream>>>((int*)ok, s, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
