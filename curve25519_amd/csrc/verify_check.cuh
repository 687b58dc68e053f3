// curve25519_amd/csrc/verify_check.cuh -- the reference-order kernels of the two-phase calls, one key per lane: what
// engine_verify.hip (the reference-order path, tables in the limb format) and engine_verify_ctx.hip (Verify_Init's canonical rows,
// the one-key kernel's lane) both instantiate.  One definition, here.
#pragma once
#include "engine_common.cuh"

// ed25519_Verify_Init (ed25519_verify.c:179-232): decompress -A (inverted parity :192-195, no validation) and
// fill the key's 16-row 4-fold table.  `tables` holds n tables of Tbl's format, `stride_words` apart.
template <typename Tbl>
__global__ void __launch_bounds__(ED_BLOCK, C25519_VI_WAVES) k_ed25519_verify_init(const void* pk, size_t n, u32* tables,
                                                                      size_t stride_words)
{
    const size_t i = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pkw[8];
    load32(pkw, pk, i);
    ge_ext Q;
    ed_decode_neg_key(Q, pkw);
    const Tbl tbl{ tables + i * stride_words };
    qtable_build(tbl, Q);
}

// ed25519_Verify_Check (ed25519_verify.c:287-313), first part: h = H(enc(R) || pk || m) mod L canonical;
// s = raw 256 bits (no s < L check, :308); T = s*B + h*(-A) projective.  The comparison with enc(R) happens in
// k_batch_invert<FinishVerify>.
template <typename Tbl>
C25519_DEV void verify_check_lane(const ProjScratch& scr, size_t n, size_t i, const void* sig, const u32 (&pkw)[8],
                                  const Msgs& msgs, const Tbl& tbl, const u32* lds_tbl)
{
    u32 Sw[8], h[8], Rw[8];
    load32(Rw, sig, 2 * i);
    ed_hram(h, Rw, pkw, msgs.ptr(i), msgs.len(i));
    sc_mod(h);
    load32(Sw, sig, 2 * i + 1);
    ge_ext T;
    ge_poly_mult(T, Sw, h, tbl, lds_tbl);
    store_proj(scr, n, i, T);
}

template <typename Tbl>
__global__ void __launch_bounds__(ED_BLOCK, C25519_VC_WAVES) k_ed25519_verify_check(ProjScratch scr, const void* sig, const void* pk,
                                                                       Msgs msgs, size_t n,
                                                                       const u32* __restrict__ g_tbl, u32* tables,
                                                                       size_t stride_words)
{
    __shared__ __attribute__((aligned(16))) u32 lds_tbl[PA_WORDS * 256];
    lds_stage_words(lds_tbl, g_tbl + REF_TBL_OFFSET, REF_TBL_WORDS);
    const size_t i = (size_t)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    u32 pkw[8];
    load32(pkw, pk, i);
    const Tbl tbl{ tables + i * stride_words };
    verify_check_lane(scr, n, i, sig, pkw, msgs, tbl, lds_tbl);
}
