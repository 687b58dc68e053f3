// curve25519_amd/csrc/engine_vrf.hip -- ed25519_VRF_Prove_*, ed25519_VRF_Verify_*, ed25519_VRF_ProofToHash_*:
// ECVRF-EDWARDS25519-SHA512-ELL2 (RFC 9381, suite string 0x04; the lane's work: vrf25519.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "vrf25519.cuh"

// One lane per element at every size, ONE kernel per call, no scratch leased: x, k and the hash prefix never leave the lane's
// registers (k's comb columns are parked in LDS, as a signing nonce's are), the points' inversions are the lane's own and shared
// between the points of an element (vrf25519.cuh), and the part of encode_to_curve's hashed string that every element shares comes
// BY VALUE in the kernel arguments (H2cTail), so a call on a capturing stream is one kernel node.  The window tables of the
// variable-base walks live in registers: two rows (width 2), the width the group calls found fastest at 2^20.
// Prove and ProofToHash run at two waves per SIMD (249 and 143 of 256 registers).  Verify keeps the points it has computed, two
// projective rows and the running point side by side: at two waves per SIMD it spilled 808 bytes a lane, at one it allocates 415 of
// 512 registers and has no scratch (tests/test_resources_vrf.py holds all three).
constexpr int VRF_BLOCK = WB_BLOCK;

// element i's 64-byte private key as vrf_prove_lane reads it: seed || public key, each half fetched where the lane asks for it
struct VrfKeyAt {
    const void* priv; size_t i;
    C25519_DEV void seed(u32 (&w)[8]) const { load32(w, priv, 2 * i); }
    C25519_DEV void pk(u32 (&w)[8]) const { load32(w, priv, 2 * i + 1); }
};

// 80-byte records as five 16-byte accesses
C25519_DEV void vrf_load_proof(u32 (&w)[VRF_PROOF_WORDS], const void* base, size_t i)
{
    const uint4* p = reinterpret_cast<const uint4*>(base) + 5 * i;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint4 a = p[j];
        w[4 * j] = a.x; w[4 * j + 1] = a.y; w[4 * j + 2] = a.z; w[4 * j + 3] = a.w;
    }
}
C25519_DEV void vrf_store_proof(void* base, size_t i, const u32 (&w)[VRF_PROOF_WORDS])
{
    uint4* p = reinterpret_cast<uint4*>(base) + 5 * i;
#pragma unroll
    for (int j = 0; j < 5; j++) p[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}
// 64-byte records as four
C25519_DEV void vrf_store_beta(void* base, size_t i, const u32 (&w)[VRF_BETA_WORDS])
{
    uint4* p = reinterpret_cast<uint4*>(base) + 4 * i;
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

__global__ void __launch_bounds__(VRF_BLOCK, 2) k_ed25519_vrf_prove(void* proof, const void* priv, const void* alpha, size_t alpha_size, size_t n,
                                                                    const u32* __restrict__ g_wide, const H2cTail tail)
{
    __shared__ unsigned short cols[WB_COLS * VRF_BLOCK];
    const size_t i = (size_t)blockIdx.x * VRF_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pi[VRF_PROOF_WORDS];
    vrf_prove_lane(pi, VrfKeyAt{ priv, i }, (const uint8_t*)alpha + i * alpha_size, tail, g_wide, cols + threadIdx.x, VRF_BLOCK);
    vrf_store_proof(proof, i, pi);
}

__global__ void __launch_bounds__(VRF_BLOCK, 1) k_ed25519_vrf_verify(void* beta, int* ok, const void* pk, const void* proof, const void* alpha,
                                                                     size_t alpha_size, size_t n, const u32* __restrict__ g_wide, const H2cTail tail)
{
    __shared__ unsigned short cols[WB_COLS * VRF_BLOCK];
    const size_t i = (size_t)blockIdx.x * VRF_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pkw[8], pi[VRF_PROOF_WORDS], b[VRF_BETA_WORDS];
    load32(pkw, pk, i);
    vrf_load_proof(pi, proof, i);
    const u32 accept = vrf_verify_lane(b, pkw, pi, (const uint8_t*)alpha + i * alpha_size, tail, g_wide, cols + threadIdx.x, VRF_BLOCK);
    vrf_store_beta(beta, i, b);
    ok[i] = accept ? 1 : 0;
}

__global__ void __launch_bounds__(VRF_BLOCK, 2) k_ed25519_vrf_proof_to_hash(void* beta, int* ok, const void* proof, size_t n)
{
    const size_t i = (size_t)blockIdx.x * VRF_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pi[VRF_PROOF_WORDS], b[VRF_BETA_WORDS];
    vrf_load_proof(pi, proof, i);
    const u32 accept = vrf_proof_to_hash_lane(b, pi);
    vrf_store_beta(beta, i, b);
    ok[i] = accept ? 1 : 0;
}

extern "C" {

// (the rules: include/curve25519_amd.h)  One lane per element at every n; c25519_amd_last_shape is not written.

int ed25519_VRF_Prove_dev(void* proof, const void* priv, const void* alpha, size_t alpha_size, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!proof || !priv || (!alpha && alpha_size)) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { proof, priv, alpha_size ? alpha : nullptr })) return rc;
    if (n == 0) return 0;
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    H2cTail tail;
    vrf_make_tail(tail, alpha_size);
    k_ed25519_vrf_prove<<<grid_for(n, VRF_BLOCK), VRF_BLOCK, 0, (hipStream_t)stream>>>(proof, priv, alpha, alpha_size, n, wide, tail);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ed25519_VRF_Verify_dev(void* beta, void* ok, const void* pk, const void* proof, const void* alpha, size_t alpha_size, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!beta || !ok || !pk || !proof || (!alpha && alpha_size)) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { beta, ok, pk, proof, alpha_size ? alpha : nullptr })) return rc;
    if (n == 0) return 0;
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    H2cTail tail;
    vrf_make_tail(tail, alpha_size);
    k_ed25519_vrf_verify<<<grid_for(n, VRF_BLOCK), VRF_BLOCK, 0, (hipStream_t)stream>>>(beta, (int*)ok, pk, proof, alpha, alpha_size, n, wide, tail);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ed25519_VRF_ProofToHash_dev(void* beta, void* ok, const void* proof, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!beta || !ok || !proof) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { beta, ok, proof })) return rc;
    if (n == 0) return 0;
    k_ed25519_vrf_proof_to_hash<<<grid_for(n, VRF_BLOCK), VRF_BLOCK, 0, (hipStream_t)stream>>>(beta, (int*)ok, proof, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
