// curve25519_amd/csrc/msm_stages.cuh -- what the two translation units that run the bucket method share: the scratch of one
// bucket-method multi-scalar multiplication as its kernels take it, and the host call that runs the stages between "every point has a
// packed row, a biased scalar and a flag" and "every window has its sum".  engine_batch_eq.hip owns the kernels (the ZIP-215 batch
// equation is their first user); engine_msm.hip (*_MultiScalarMult_vartime_*) runs them over points that all have a scalar of their own.
#pragma once
#include "engine_common.cuh"
#include "msm25519.cuh"

// scratch of one equation, cut from the calling thread's slab (batcheq_layout): n elements, N = 2n points (keys, then R's),
// K = (wa + 1) * buckets counters (the windows of buckets: msm25519.cuh, MsmShape)
struct BatchEqScratch {
    u32* rows;              // [N][32]  packed row of -P (msm_point_row), 128-byte aligned
    u32* buckets;           // [K][40]  bucket sums
    u32* windows;           // [wa + 1][40] window sums
    u32* sc;                // [8][N]   biased scalars, word-major: a_i for key i, z_i for R i
    u32* entries;           // [n (wa + wz)] the inverted index: point * 2 + sign, grouped by (window, bucket)
    u32* partial;           // [blocks][16] per-workgroup sums of the s_i, in 16-bit chunks
    u32* flags;             // [n]      non-zero: the element is left out (S >= L, a key or an R that does not decode)
    u32* counts;            // [K]      entries per (window, bucket)
    u32* cursor;            // [K]      where the bucket's list begins; after the scatter, where it ends
    u32* reject;            // [1]      non-zero: some element was left out -> result 0
};
typedef MsmShape BatchEqShape;                               // (msm25519.cuh)

namespace c25519_engine {

// (engine_batch_eq.hip) count, scan, scatter, buckets, windows -- the coalesced equation's kernels as they are -- over N points that are
// all "keys": point p has the biased scalar sc[.][p] (below L before the bias), the row rows[p] and the flag flags[p] (non-zero: it is
// left out); there are no R points and window wa stays empty, so K = wa * buckets counters and wa window sums are used.  flags (where a
// point is kept) and counts must be zero.  Leaves windows[0 .. wa - 1]; one equation takes at most 2^26 points.
int batcheq_bucket_stages(const BatchEqScratch& s, size_t N, const BatchEqShape& sh, hipStream_t stream);

}  // namespace c25519_engine
