// curve25519_amd/csrc/engine_keys.hip -- ed25519_ClassifyKey_*, ed25519_PublicKey_to_X25519_*, ed25519_PrivateKey_to_X25519_*: key
// classification and conversion to X25519 keys (the lane's work: ed_keys.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "ed_keys.cuh"

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

extern "C" {

// (the rules: include/curve25519_amd.h)  One lane per key at every n; c25519_amd_last_shape is not written.

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
    ProjScratch scr;                                          // a = 1 + y, z = 1 - y, b = the ok words (n of its 10 n)
    c25519_host::WorkLease lease;
    C25519_RC(lease_proj(&scr, lease, n, stream));
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
