// curve25519_amd/csrc/engine_oprf.hip -- ristretto255_OPRF_Blind_*, ristretto255_OPRF_Finalize_*, ristretto255_OPRF_BlindEvaluate_*,
// ristretto255_VOPRF_BlindEvaluate_*, ristretto255_VOPRF_VerifyProof_*: RFC 9497's OPRF (mode 0x00) and VOPRF (mode 0x01) with
// ciphersuite ristretto255-SHA512 (the lane's work: oprf25519.cuh) -- kernels and *_dev entry points
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"
#include "oprf25519.cuh"

// The three per-row calls are ONE kernel each, one lane per row, no scratch leased: the hashed element goes from the Elligator sum
// into the walk in registers, Finalize's inversion mod L and its hash are the lane's own, and the server's ONE key is read by every
// lane from its 32 bytes of device memory (a uniform address).  Blind takes the uniform part of HashToGroup's string BY VALUE
// (H2cTail), as the hashing calls do.
// The two proof calls are three stages on the caller's stream over one lease of scratch (oprf_layout):
//   (a) k_oprf_server_head / k_oprf_verifier_head, ONE lane: pkS (the server's: [skS]B over the wide comb) and the composites' seed
//       into the scratch's header;
//   (b) k_oprf_server_rows / k_oprf_verifier_rows, one lane per row: the row's request by bisection over `offsets`, D_i = [skS]C_i
//       (the server), d_i, and [d_i]C_i as an extended point into scratch, with the request's number where the row is accepted (the
//       verifier: a second lane per row does the same for [d_i]D_i);
//   (c) k_oprf_prove / k_oprf_check, one lane per request: the sum of its rows' points, the walks, four encodings, the challenge.
// Nothing is allocated beyond the lease and no stage reads anything back, so a call on a capturing stream is three kernel nodes.
// skS and proof_rand are read from device memory where they are used: they are never kernel arguments.
// Stage (c) sums a request's rows in ONE lane: a proof over tens of thousands of rows is that many dependent additions in a single
// lane (profiles/oprf_rate.txt), the price of requests that need nothing from each other.  Calls of many small requests, what an
// issuer sees, keep every lane busy.
constexpr int OPRF_BLOCK = WB_BLOCK;
constexpr int OPRF_REQ_BLOCK = 64;                           // stage (c): one wave a workgroup, the whole register file of a SIMD's lane

// 64-byte records as four 16-byte accesses
C25519_DEV void oprf_load64(u32 (&w)[16], const void* base, size_t i)
{
    const uint4* p = reinterpret_cast<const uint4*>(base) + 4 * i;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 a = p[j];
        w[4 * j] = a.x; w[4 * j + 1] = a.y; w[4 * j + 2] = a.z; w[4 * j + 3] = a.w;
    }
}
C25519_DEV void oprf_store64(void* base, size_t i, const u32 (&w)[16])
{
    uint4* p = reinterpret_cast<uint4*>(base) + 4 * i;
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}

__global__ void __launch_bounds__(OPRF_BLOCK, 2) k_oprf_blind(void* blinded, int* ok, const void* input, size_t input_size, const void* blind, size_t n,
                                                              const H2cTail tail)
{
    const size_t i = (size_t)blockIdx.x * OPRF_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 bw[8], out[8];
    load32(bw, blind, i);
    const u32 accept = oprf_blind_lane(out, (const uint8_t*)input + i * input_size, tail, bw);
    store32(blinded, i, out);
    ok[i] = (int)(accept & 1u);
}

__global__ void __launch_bounds__(OPRF_BLOCK, 2) k_oprf_finalize(void* output, int* ok, const void* input, size_t input_size, const void* blind,
                                                                 const void* evaluated, size_t n)
{
    const size_t i = (size_t)blockIdx.x * OPRF_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 bw[8], ew[8], out[16];
    load32(bw, blind, i);
    load32(ew, evaluated, i);
    const u32 accept = oprf_finalize_lane(out, (const uint8_t*)input + i * input_size, input_size, bw, ew);
    oprf_store64(output, i, out);
    ok[i] = (int)(accept & 1u);
}

__global__ void __launch_bounds__(OPRF_BLOCK, 2) k_oprf_evaluate(void* evaluated, int* ok, const void* sks, const void* blinded, size_t n)
{
    const size_t i = (size_t)blockIdx.x * OPRF_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 kw[8], pw[8], out[8];
    load32(kw, sks, 0);
    load32(pw, blinded, i);
    const u32 accept = oprf_evaluate_lane(out, kw, pw);
    store32(evaluated, i, out);
    ok[i] = (int)(accept & 1u);
}

// ---- the proof calls -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64, 1) k_oprf_server_head(u32* head, const void* sks, const u32* __restrict__ g_wide)
{
    __shared__ unsigned short cols[WB_COLS];
    if (blockIdx.x || threadIdx.x) return;
    u32 kw[8];
    load32(kw, sks, 0);
    OprfHead h;
    oprf_server_head_lane(h, kw, g_wide, cols, 1);
    oprf_store_head(head, h);
}

__global__ void __launch_bounds__(64, 1) k_oprf_verifier_head(u32* head, const void* pks)
{
    if (blockIdx.x || threadIdx.x) return;
    u32 pw[8];
    load32(pw, pks, 0);
    OprfHead h;
    oprf_verifier_head_lane(h, pw);
    oprf_store_head(head, h);
}

__global__ void __launch_bounds__(OPRF_BLOCK, 2) k_oprf_server_rows(void* evaluated, int* ok, OprfPoints pts, u32* owner, const u32* head, const void* sks,
                                                                    const void* blinded, const unsigned long long* offsets, size_t m, size_t n)
{
    const size_t i = (size_t)blockIdx.x * OPRF_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 idx;
    const u32 j = oprf_owner(idx, offsets, m, n, i);
    u32 kw[8], Dw[8];
    load32(kw, sks, 0);
    ge_ext term;
    const u32 accept = oprf_server_row_lane(Dw, term, kw, [&](u32 (&w)[8]) { load32(w, blinded, i); }, [&](u64 (&seed)[8]) { oprf_load_seed(seed, head); },
                                            idx, j == OPRF_NO_OWNER ? 0u : 0xffffffffu);
    store32(evaluated, i, Dw);
    ok[i] = (int)(accept & 1u);
    oprf_store_point(pts, n, i, term);
    owner[i] = (j & accept) | ~accept;
}

// 2 n lanes: lane i takes [d_i]C_i, lane n + i takes [d_i]D_i
__global__ void __launch_bounds__(OPRF_BLOCK, 2) k_oprf_verifier_rows(OprfPoints pts_c, OprfPoints pts_d, u32* owner_c, u32* owner_d, const u32* head,
                                                                      const void* blinded, const void* evaluated, const unsigned long long* offsets, size_t m,
                                                                      size_t n)
{
    const size_t lane = (size_t)blockIdx.x * OPRF_BLOCK + threadIdx.x;
    if (lane >= 2 * n) return;
    const bool second = lane >= n;
    const size_t i = second ? lane - n : lane;
    u32 idx;
    const u32 j = oprf_owner(idx, offsets, m, n, i);
    ge_ext term;
    const u32 accept = oprf_verifier_point_lane(term, [&](u32 k, u32 (&w)[8]) { load32(w, k ? evaluated : blinded, i); },
                                                [&](u64 (&seed)[8]) { oprf_load_seed(seed, head); }, idx, j == OPRF_NO_OWNER ? 0u : 0xffffffffu,
                                                second ? 0xffffffffu : 0u);
    oprf_store_point(second ? pts_d : pts_c, n, i, term);
    (second ? owner_d : owner_c)[i] = (j & accept) | ~accept;
}

__global__ void __launch_bounds__(OPRF_REQ_BLOCK, 1) k_oprf_prove(void* proof, int* req_ok, OprfPoints pts, const u32* owner, const u32* head, const void* sks,
                                                                  const void* proof_rand, const unsigned long long* offsets, size_t m, size_t n,
                                                                  const u32* __restrict__ g_wide)
{
    __shared__ unsigned short cols[WB_COLS * OPRF_REQ_BLOCK];
    const size_t j = (size_t)blockIdx.x * OPRF_REQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    size_t lo;
    u32 count;
    u32 good = oprf_request(lo, count, offsets, j, n) ? 0xffffffffu : 0u;
    ge_ext M;
    good &= oprf_sum_rows(M, pts, owner, n, lo, count, (u32)j);
    OprfHead h;
    oprf_load_head(h, head);
    u32 kw[8], rw[8], pf[16];
    load32(kw, sks, 0);
    load32(rw, proof_rand, j);
    const u32 accept = oprf_prove_lane(pf, M, kw, rw, h, good, g_wide, cols + threadIdx.x, OPRF_REQ_BLOCK);
    oprf_store64(proof, j, pf);
    req_ok[j] = (int)(accept & 1u);
}

__global__ void __launch_bounds__(OPRF_REQ_BLOCK, 1) k_oprf_check(int* req_ok, OprfPoints pts_c, OprfPoints pts_d, const u32* owner_c, const u32* owner_d,
                                                                  const u32* head,
                                                                  const void* proof, const unsigned long long* offsets, size_t m, size_t n,
                                                                  const u32* __restrict__ g_wide)
{
    __shared__ unsigned short cols[WB_COLS * OPRF_REQ_BLOCK];
    const size_t j = (size_t)blockIdx.x * OPRF_REQ_BLOCK + threadIdx.x;
    if (j >= m) return;
    size_t lo;
    u32 count;
    u32 good = oprf_request(lo, count, offsets, j, n) ? 0xffffffffu : 0u;
    ge_ext M, Z;
    good &= oprf_sum_rows(M, pts_c, owner_c, n, lo, count, (u32)j);
    good &= oprf_sum_rows(Z, pts_d, owner_d, n, lo, count, (u32)j);
    OprfHead h;
    oprf_load_head(h, head);
    u32 pf[16];
    oprf_load64(pf, proof, j);
    const u32 accept = oprf_check_lane(M, Z, pf, h, good, g_wide, cols + threadIdx.x, OPRF_REQ_BLOCK);
    req_ok[j] = (int)(accept & 1u);
}

namespace {

// the scratch of a proof call: `sums` extended points a row (the server's [d_i]C_i; the verifier's [d_i]D_i too), for each of them the
// request that owns the accepted row, the call's header
struct OprfScratch { OprfPoints c, d; u32 *owner, *owner_d, *head; };
OprfScratch oprf_layout(Carve& cv, size_t n, int sums)
{
    OprfScratch s;
    auto points = [&](size_t rows) {
        OprfPoints p;
        p.X = cv.take4(SCR_FE * rows);
        p.Y = cv.take4(SCR_FE * rows);
        p.Z = cv.take4(SCR_FE * rows);
        p.T = cv.take4(SCR_FE * rows);
        return p;
    };
    s.c = points(n);
    s.d = points(sums > 1 ? n : 0);
    s.owner = cv.take4(n);
    s.owner_d = cv.take4(sums > 1 ? n : 0);
    s.head = cv.take4(OPRF_HEAD_WORDS);
    return s;
}

int oprf_check_proof_args(size_t m, size_t n)
{
    if (m > ((size_t)1 << 31)) return bad_arg("too many requests (m > 2^31)");
    if (n > ((size_t)1 << 31)) return bad_arg("batch too large (n > 2^31)");
    return 0;
}

}  // namespace

extern "C" {

// (the rules: include/curve25519_amd.h)  One lane per row or per request at every size; c25519_amd_last_shape is not written.

size_t ristretto255_VOPRF_scratch_bytes(size_t m, size_t n)
{
    (void)m;                                                 // (a request leaves nothing in scratch: its lane holds its sums)
    return layout_bytes([n](Carve& c) { return oprf_layout(c, n, 2); });
}

int ristretto255_OPRF_Blind_dev(void* blinded, void* ok, const void* input, size_t input_size, const void* blind, int mode, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!blinded || !ok || !blind || (!input && input_size)) return bad_arg("null pointer");
    if (mode != 0 && mode != 1) return bad_arg("mode must be 0 (OPRF) or 1 (VOPRF)");
    if (input_size > 65535) return bad_arg("input_size must be at most 65535");
    if (int rc = check_dev_args(n, { blinded, ok, input_size ? input : nullptr, blind })) return rc;
    if (n == 0) return 0;
    H2cTail tail;
    oprf_make_tail(tail, input_size, (unsigned)mode);
    k_oprf_blind<<<grid_for(n, OPRF_BLOCK), OPRF_BLOCK, 0, (hipStream_t)stream>>>(blinded, (int*)ok, input, input_size, blind, n, tail);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ristretto255_OPRF_Finalize_dev(void* output, void* ok, const void* input, size_t input_size, const void* blind, const void* evaluated, size_t n,
                                   void* stream)
{
    C25519_API_CALL();
    if (!output || !ok || !blind || !evaluated || (!input && input_size)) return bad_arg("null pointer");
    if (input_size > 65535) return bad_arg("input_size must be at most 65535");
    if (int rc = check_dev_args(n, { output, ok, input_size ? input : nullptr, blind, evaluated })) return rc;
    if (n == 0) return 0;
    k_oprf_finalize<<<grid_for(n, OPRF_BLOCK), OPRF_BLOCK, 0, (hipStream_t)stream>>>(output, (int*)ok, input, input_size, blind, evaluated, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ristretto255_OPRF_BlindEvaluate_dev(void* evaluated, void* ok, const void* skS, const void* blinded, size_t n, void* stream)
{
    C25519_API_CALL();
    if (!evaluated || !ok || !skS || !blinded) return bad_arg("null pointer");
    if (int rc = check_dev_args(n, { evaluated, ok, skS, blinded })) return rc;
    if (n == 0) return 0;
    k_oprf_evaluate<<<grid_for(n, OPRF_BLOCK), OPRF_BLOCK, 0, (hipStream_t)stream>>>(evaluated, (int*)ok, skS, blinded, n);
    C25519_TRY(hipGetLastError());
    return 0;
}

int ristretto255_VOPRF_BlindEvaluate_dev(void* evaluated, void* proof, void* ok, void* req_ok, const void* skS, const void* proof_rand,
                                         const void* blinded, const void* offsets, size_t m, size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!skS || !offsets || (n && (!evaluated || !ok || !blinded)) || (m && (!proof || !req_ok || !proof_rand))) return bad_arg("null pointer");
    if (int rc = oprf_check_proof_args(m, n)) return rc;
    if (int rc = check_dev_args(n, { evaluated, ok, blinded })) return rc;
    if (int rc = check_dev_args(std::max(m, n), { proof, req_ok, skS, proof_rand, offsets })) return rc;
    if (n == 0 && m == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    OprfScratch s;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&s, lease, stream, [n](Carve& c) { return oprf_layout(c, n, 1); }));
    const unsigned long long* off = (const unsigned long long*)offsets;
    k_oprf_server_head<<<1, 64, 0, stream>>>(s.head, skS, wide);
    C25519_TRY(hipGetLastError());
    if (n) {
        k_oprf_server_rows<<<grid_for(n, OPRF_BLOCK), OPRF_BLOCK, 0, stream>>>(evaluated, (int*)ok, s.c, s.owner, s.head, skS, blinded, off, m, n);
        C25519_TRY(hipGetLastError());
    }
    if (m) {
        k_oprf_prove<<<grid_for(m, OPRF_REQ_BLOCK), OPRF_REQ_BLOCK, 0, stream>>>(proof, (int*)req_ok, s.c, s.owner, s.head, skS, proof_rand, off, m, n, wide);
        C25519_TRY(hipGetLastError());
    }
    return lease.release();
}

int ristretto255_VOPRF_VerifyProof_dev(void* req_ok, const void* pkS, const void* blinded, const void* evaluated, const void* proof, const void* offsets,
                                       size_t m, size_t n, void* stream_)
{
    C25519_API_CALL();
    if (!pkS || !offsets || (n && (!blinded || !evaluated)) || (m && (!req_ok || !proof))) return bad_arg("null pointer");
    if (int rc = oprf_check_proof_args(m, n)) return rc;
    if (int rc = check_dev_args(n, { blinded, evaluated })) return rc;
    if (int rc = check_dev_args(std::max(m, n), { req_ok, pkS, proof, offsets })) return rc;
    if (m == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    const u32* wide = nullptr;
    C25519_RC(wide_tables(&wide));
    OprfScratch s;
    c25519_host::WorkLease lease;
    C25519_RC(lease_scratch(&s, lease, stream, [n](Carve& c) { return oprf_layout(c, n, 2); }));
    const unsigned long long* off = (const unsigned long long*)offsets;
    k_oprf_verifier_head<<<1, 64, 0, stream>>>(s.head, pkS);
    C25519_TRY(hipGetLastError());
    if (n) {
        k_oprf_verifier_rows<<<grid_for(2 * n, OPRF_BLOCK), OPRF_BLOCK, 0, stream>>>(s.c, s.d, s.owner, s.owner_d, s.head, blinded, evaluated, off, m, n);
        C25519_TRY(hipGetLastError());
    }
    k_oprf_check<<<grid_for(m, OPRF_REQ_BLOCK), OPRF_REQ_BLOCK, 0, stream>>>((int*)req_ok, s.c, s.d, s.owner, s.owner_d, s.head, proof, off, m, n, wide);
    C25519_TRY(hipGetLastError());
    return lease.release();
}

}  // extern "C"
