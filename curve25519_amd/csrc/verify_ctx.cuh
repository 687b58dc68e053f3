// curve25519_amd/csrc/verify_ctx.cuh -- ed25519_Verify_Check against MANY contexts in one call (ed25519_Verify_Check_indexed_*):
// element i is checked against context ctx_index[i] of the call's n_ctx 2080-byte records (Verify_Init's layout: pk || 16 rows of
// four canonical field elements, read as they are, like the reference: ed25519_verify.c:287-313).  The lane's work is
// verify_check_lane's (verify_check.cuh) with the key and the rows taken from the element's own context; the comparison with
// enc(R) happens in k_batch_invert<FinishVerifyIndexed>.  In a header of its own so that tests/host_emul compiles it too.
//
// The index is public data (which key a signature claims), so its gather and bounds check take no constant-time care.  An index
// >= n_ctx reads nothing: its lane leaves the zero point and the finish writes verdict 0 from the index itself.  (The zero point
// alone would not do: the inversion maps Z = 0 to 0, enc(T) would be 32 zero bytes, and an R of 32 zero bytes would pass.)
#pragma once
#include "lanes.cuh"
#include "ge25519.cuh"

#ifndef C25519_INDEXED_REPACK
#define C25519_INDEXED_REPACK 0      // A/B switch: 1 = copy the call's rows into 128-byte-aligned rows of work scratch first
#endif                               // (k_ed25519_verify_ctx_repack); 0 = read them where they are (profiles/indexed_check_rate.txt)

namespace c25519 {

constexpr size_t VCTX_BYTES = 2080, VCTX_WORDS = VCTX_BYTES / 4;

// element i's context, or null when its index is out of range
C25519_DEV const u32* indexed_ctx(const u32* ctxs, size_t n_ctx, const u32* ctx_index, size_t i)
{
    const u32 k = ctx_index[i];
    return k < n_ctx ? ctxs + (size_t)k * VCTX_WORDS : nullptr;
}

// T = s*B + h*(-A) of element i against context `ctx`, its 16 rows read through `tbl` (the context's own rows, QTableCanon{ ctx + 8 },
// or a copy of them); the zero point when ctx is null
template <typename Tbl>
C25519_DEV void verify_ctx_point(ge_ext& T, const u32* ctx, const Tbl& tbl, const void* sig, const Msgs& msgs, size_t i,
                                 const u32* lds_tbl)
{
    if (!ctx) {
        fe_set_u32(T.X, 0); fe_set_u32(T.Y, 0); fe_set_u32(T.Z, 0); fe_set_u32(T.T, 0);
        return;
    }
    u32 pkw[8], Sw[8], h[8], Rw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pkw[j] = ctx[j];
    load32(Rw, sig, 2 * i);
    ed_hram(h, Rw, pkw, msgs.ptr(i), msgs.len(i));
    sc_mod(h);
    load32(Sw, sig, 2 * i + 1);                            // raw 256 bits: no s < L check (ed25519_verify.c:308)
    ge_poly_mult(T, Sw, h, tbl, lds_tbl);
}

// verdict = (enc(T) == enc(R) bytes) and the element's index in range   (ed25519_verify.c:310-312)
struct FinishVerifyIndexed {
    const u32 *X, *Y; const void* sig; int* verdict; size_t n;
    const u32* ctx_index; size_t n_ctx;
    C25519_DEV bool skip() const { return false; }
    C25519_DEV void emit(size_t e, const fe& zinv) const
    {
        fe t;
        u32 xw[8], yw[8], enc[8], Rw[8];
        soa_load_fe(t, X, n, e);  fe_mul(t, t, zinv);  fe_to_words(xw, t);
        soa_load_fe(t, Y, n, e);  fe_mul(t, t, zinv);  fe_to_words(yw, t);
        ge_pack(enc, xw, yw);
        load32(Rw, sig, 2 * e);
        u32 diff = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) diff |= enc[j] ^ Rw[j];
        verdict[e] = (diff == 0 && ctx_index[e] < n_ctx) ? 1 : 0;
    }
};

}  // namespace c25519
