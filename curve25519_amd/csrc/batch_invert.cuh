// curve25519_amd/csrc/batch_invert.cuh -- what the shared inversion (k_batch_invert, engine_common.cuh; Montgomery's trick over K
// elements per lane, one inversion per quad of lanes: one per lane lost, profiles/r06_ab_inv_quad.txt) is made of, in a header that tests/host_emul compiles too: its group sizes, the
// zero swap, the LDS moves and the self-test's output.  The lane's work itself is batch_invert_lane.inc (see there why).
#pragma once
#include "lanes.cuh"
#include "quad25519.cuh"

namespace c25519 {

constexpr int INV_BLOCK = 64;
constexpr int INV_MAX_K = 16;

// the group sizes k_batch_invert is instantiated for: a request of k elements per lane rounds down to one of them
inline int inversion_group(long k)
{
    return k >= 16 ? 16 : k >= 14 ? 14 : k >= 12 ? 12 : k >= 8 ? 8 : k >= 4 ? 4 : k >= 2 ? 2 : 1;
}

C25519_DEV void lds_put_fe(u32* buf, int stride, int idx, const fe& f)
{
#pragma unroll
    for (int w = 0; w < 10; w++) buf[w * stride + idx] = f.v[w];
}
C25519_DEV void lds_get_fe(fe& f, const u32* buf, int stride, int idx)
{
#pragma unroll
    for (int w = 0; w < 10; w++) f.v[w] = buf[w * stride + idx];
}

// z <- 1 where z == 0 (mod p), returns all-ones in that case: a zero takes no part in a shared inversion and its
// "inverse" is forced to 0 afterwards, which is what the reference's z^(p-2) gives (curve25519_dh.c:148)
C25519_DEV u32 fe_zero_to_one(fe& z)
{
    u32 w[8], nz = 0;
    fe_to_words(w, z);
#pragma unroll
    for (int q = 0; q < 8; q++) nz |= w[q];
    const u32 is_zero = nz ? 0u : 0xffffffffu;
    fe one;
    fe_set_u32(one, 1);
    fe_select(z, is_zero, one, z);
    return is_zero;
}

// the self-test's output: the canonical words of each 1 / z, 32 bytes per element (c25519_amd_batch_invert_selftest_dev)
struct FinishInverse {
    u32* out;
    C25519_DEV bool skip() const { return false; }
    C25519_DEV void emit(size_t e, const fe& zinv) const
    {
        u32 w[8];
        fe_to_words(w, zinv);
        store32(out, e, w);
    }
};

}  // namespace c25519
