// tests/ct_probe.hip -- TEST INFRASTRUCTURE.  Two kernels with a known answer for tests/test_gpu_secret_counts.py, which holds that
// the instruction counts of the product's kernels do not move with their secrets: k_ct_probe_branch does extra multiplications
// under `if (secret & 1)`, so its VALU instruction count must differ between all-zero and all-ones input; k_ct_probe_select does the
// same work for every lane and picks by mask, so its count must not.  k_ct_marker separates the calls in the profiler's dispatch
// list.  Compiled by tests/secret_counts_child.py into a temporary directory; not part of the product.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int ROUNDS = 64;

__device__ __forceinline__ uint32_t extra_work(uint32_t x)
{
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) x = x * (x | 1u) + 0x7F4A7C15u;       // (not affine: the compiler cannot fold the rounds)
    return x;
}

}  // namespace

__global__ void k_ct_probe_branch(uint32_t* out, const uint32_t* secret, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i | 1u;
    if (secret[i] & 1u) x = extra_work(x);
    out[i] = x;
}

__global__ void k_ct_probe_select(uint32_t* out, const uint32_t* secret, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = (uint32_t)i | 1u, y = extra_work(x), m = 0u - (secret[i] & 1u);
    out[i] = (y & m) | (x & ~m);
}

__global__ void k_ct_marker(uint32_t* count)
{
    if (threadIdx.x == 0) count[0] += 1u;
}

extern "C" int ct_probe_launch(int select, void* out, const void* secret, size_t n, void* stream)
{
    const unsigned block = 256, grid = (unsigned)((n + block - 1) / block);
    if (select) k_ct_probe_select<<<grid, block, 0, (hipStream_t)stream>>>((uint32_t*)out, (const uint32_t*)secret, n);
    else k_ct_probe_branch<<<grid, block, 0, (hipStream_t)stream>>>((uint32_t*)out, (const uint32_t*)secret, n);
    return (int)hipGetLastError();
}

extern "C" int ct_marker_launch(void* count, void* stream)
{
    k_ct_marker<<<1, 64, 0, (hipStream_t)stream>>>((uint32_t*)count);
    return (int)hipGetLastError();
}
