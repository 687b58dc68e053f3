// curve25519_amd/csrc/engine_h2c.hip -- c25519_ExpandMessageXmd_*, ed25519_MapToCurve_*, ed25519_HashToCurve_*,
// ed25519_EncodeToCurve_*, ristretto255_HashToGroup_*, ed25519_HashToScalar_*: hashing messages to edwards25519, ristretto255 and
// the scalar field (RFC 9380, RFC 9497; the lane's work: h2c25519.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "h2c25519.cuh"

// One lane per element at every size, ONE kernel per call, two waves per SIMD (256 registers a lane), no scratch leased.  The part
// of the hashed strings that is the same for every element -- the lengths, the DST, the padding -- comes BY VALUE in the kernel
// arguments (H2cTail, h2c25519.cuh): the DST is a host pointer, nothing is allocated or copied on the stream, and a call on a
// capturing stream is one kernel node.
// The Edwards encoding's inversion is the lane's own (fe_invert, the division steps: ~16 000 instructions behind two ~25 000
// instruction square-root chains and five compressions) and NOT the shared k_batch_invert: sharing it would cost a scratch lease of
// 160 bytes an element, a second launch and a round trip through memory to save at most a fifth of the lane's work, and the
// compiler's remarks leave room for it -- with the inversion in the lane k_h2c_to_curve<2> allocates 212 of the 256 registers its
// launch bounds give it, k_h2c_to_curve<1> and k_h2c_map 168, and none has scratch (tests/test_resources_h2c.py holds both).
constexpr int H2C_BLOCK = 256;

__global__ void __launch_bounds__(H2C_BLOCK, 2) k_h2c_expand(void* out, const void* msg, size_t msg_size, size_t n, const H2cTail tail)
{
    const size_t i = (size_t)blockIdx.x * H2C_BLOCK + threadIdx.x;
    if (i >= n) return;
    h2c_expand_lane((uint8_t*)out + i * tail.len_in_bytes, (const uint8_t*)msg + i * msg_size, tail);
}

__global__ void __launch_bounds__(H2C_BLOCK, 2) k_h2c_map(void* p, const void* u, size_t n)
{
    const size_t i = (size_t)blockIdx.x * H2C_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 uw[8], out[8];
    load32(uw, u, i);
    h2c_map_lane(out, uw);
    store32(p, i, out);
}

// COUNT = 2: HashToCurve (..._RO_), 1: EncodeToCurve (..._NU_)
template <int COUNT>
__global__ void __launch_bounds__(H2C_BLOCK, 2) k_h2c_to_curve(void* p, const void* msg, size_t msg_size, size_t n, const H2cTail tail)
{
    const size_t i = (size_t)blockIdx.x * H2C_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 out[8];
    h2c_to_curve_lane<COUNT>(out, (const uint8_t*)msg + i * msg_size, tail);
    store32(p, i, out);
}

__global__ void __launch_bounds__(H2C_BLOCK, 2) k_h2c_to_group(void* p, const void* msg, size_t msg_size, size_t n, const H2cTail tail)
{
    const size_t i = (size_t)blockIdx.x * H2C_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 out[8];
    h2c_to_group_lane(out, (const uint8_t*)msg + i * msg_size, tail);
    store32(p, i, out);
}

__global__ void __launch_bounds__(H2C_BLOCK, 2) k_h2c_to_scalar(void* s, const void* msg, size_t msg_size, size_t n, const H2cTail tail)
{
    const size_t i = (size_t)blockIdx.x * H2C_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 out[8];
    h2c_to_scalar_lane(out, (const uint8_t*)msg + i * msg_size, tail);
    store32(s, i, out);
}

namespace c25519_engine {

// the argument rules every call of this unit shares (include/curve25519_amd.h): 0, or the error already noted
int h2c_check_args(const void* out, const void* msg, size_t msg_size, const void* dst, size_t dst_len, size_t len_in_bytes)
{
    if (!out || !dst || (!msg && msg_size)) return bad_arg("null pointer");
    if (dst_len < 1 || dst_len > (size_t)H2C_MAX_DST) return bad_arg("dst_len must be 1 .. 255 (the oversize-DST rule is not implemented)");
    if (len_in_bytes < 1 || len_in_bytes > (size_t)H2C_MAX_LEN) return bad_arg("len_in_bytes must be 1 .. 16320");
    return 0;
}

}  // namespace c25519_engine

namespace {

enum H2cCall { H2C_HASH_TO_CURVE, H2C_ENCODE_TO_CURVE, H2C_TO_GROUP, H2C_TO_SCALAR };

// the four calls that write 32 bytes an element
int h2c_point_dev(H2cCall call, void* p, const void* msg, size_t msg_size, const void* dst, size_t dst_len, size_t n, void* stream_)
{
    C25519_API_CALL();
    if (int rc = h2c_check_args(p, msg, msg_size, dst, dst_len, 64)) return rc;
    if (int rc = check_dev_args(n, { p, msg_size ? msg : nullptr })) return rc;
    if (n == 0) return 0;
    H2cTail tail;
    h2c_make_tail(tail, msg_size, (const unsigned char*)dst, dst_len, call == H2C_HASH_TO_CURVE ? 96 : call == H2C_ENCODE_TO_CURVE ? 48 : 64);
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned grid = grid_for(n, H2C_BLOCK);
    switch (call) {
        case H2C_HASH_TO_CURVE:   k_h2c_to_curve<2><<<grid, H2C_BLOCK, 0, stream>>>(p, msg, msg_size, n, tail); break;
        case H2C_ENCODE_TO_CURVE: k_h2c_to_curve<1><<<grid, H2C_BLOCK, 0, stream>>>(p, msg, msg_size, n, tail); break;
        case H2C_TO_GROUP:        k_h2c_to_group<<<grid, H2C_BLOCK, 0, stream>>>(p, msg, msg_size, n, tail); break;
        default:                  k_h2c_to_scalar<<<grid, H2C_BLOCK, 0, stream>>>(p, msg, msg_size, n, tail); break;
    }
    C25519_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

// (the rules: include/curve25519_amd.h)  One lane per element at every n; c25519_amd_last_shape is not written.

int c25519_ExpandMessageXmd_dev(void* out, const void* msg, size_t msg_size, const void* dst, size_t dst_len, size_t len_in_bytes, size_t n,
                                void* stream)
{
    C25519_API_CALL();
    if (int rc = h2c_check_args(out, msg, msg_size, dst, dst_len, len_in_bytes)) return rc;
    if (int rc = check_dev_args(n, { out, msg_size ? msg : nullptr })) return rc;
    if (n == 0) return 0;
    H2cTail tail;
    h2c_make_tail(tail, msg_size, (const unsigned char*)dst, dst_len, len_in_bytes);
    k_h2c_expand<<<grid_for(n, H2C_BLOCK), H2C_BLOCK, 0, (hipStream_t)stream>>>(out, msg, msg_size, n, tail);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ed25519_MapToCurve_dev(void* p, const void* u, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!p || !u) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { p, u })) return rc;
    if (n == 0) return 0;
    k_h2c_map<<<grid_for(n, H2C_BLOCK), H2C_BLOCK, 0, (hipStream_t)stream>>>(p, u, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ed25519_HashToCurve_dev(void* p, const void* msg, size_t msg_size, const void* dst, size_t dst_len, size_t n, void* stream)
{
    return h2c_point_dev(H2C_HASH_TO_CURVE, p, msg, msg_size, dst, dst_len, n, stream);
}

int ed25519_EncodeToCurve_dev(void* p, const void* msg, size_t msg_size, const void* dst, size_t dst_len, size_t n, void* stream)
{
    return h2c_point_dev(H2C_ENCODE_TO_CURVE, p, msg, msg_size, dst, dst_len, n, stream);
}

int ristretto255_HashToGroup_dev(void* p, const void* msg, size_t msg_size, const void* dst, size_t dst_len, size_t n, void* stream)
{
    return h2c_point_dev(H2C_TO_GROUP, p, msg, msg_size, dst, dst_len, n, stream);
}

int ed25519_HashToScalar_dev(void* s, const void* msg, size_t msg_size, const void* dst, size_t dst_len, size_t n, void* stream)
{
    return h2c_point_dev(H2C_TO_SCALAR, s, msg, msg_size, dst, dst_len, n, stream);
}

}  // extern "C"
