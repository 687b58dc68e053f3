// curve25519_amd/csrc/strict25519.cuh -- the input rules of the strict verification calls (ed25519_VerifySignature_strict_*,
// ed25519_Verify_Check_strict_*; include/curve25519_amd.h states them), as branch-free predicates over 8 little-endian words.
// Every result is all-ones or zero.  The lane, quad and per-wave kernels include this header, and so does the CPU emulator
// (tests/host_emul/verify_strict.cpp).
//   rule 1   S < L
//   rule 2   y_A < p                    (bit 255 cleared: the sign of x)
//   rule 3   y_A mod p not the y of a point of small order
//   rule 5   y_R mod p not the y of a point of small order (any 255-bit value: p and p + 1 count)
// Rule 4 (the key decodes onto the curve) is the square root the kernels take anyway; rule 6 is the plain call's verdict.
#pragma once
#include "curve_constants.cuh"

namespace c25519 {

// a < b as 256-bit integers
C25519_DEV u32 strict_less(const u32 (&a)[8], const u32 (&b)[8])
{
    u32 borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) borrow = (u32)((((u64)a[i] - b[i]) - borrow) >> 63);
    return 0u - borrow;
}

// y (bit 255 ignored) mod p is 0, 1, p - 1 or the y of a point of order 8
C25519_DEV u32 strict_small_y(const u32 (&w)[8])
{
    u32 any = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        u32 diff = (w[7] & 0x7fffffffu) ^ K_SMALL_Y[k][7];
#pragma unroll
        for (int i = 0; i < 7; i++) diff |= w[i] ^ K_SMALL_Y[k][i];
        any |= diff == 0 ? 1u : 0u;
    }
    return 0u - any;
}

// rules 1 and 5, what the scalar step of an element decides: all-ones if the pair is rejected
C25519_DEV u32 strict_reject_pair(const u32 (&Rw)[8], const u32 (&Sw)[8])
{
    return ~strict_less(Sw, K_L) | strict_small_y(Rw);
}

// rules 2 and 3 on the key's bytes: all-ones if the key is rejected (rule 4 is the caller's square root)
C25519_DEV u32 strict_reject_key(const u32 (&w)[8])
{
    u32 y[8];
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = w[i];
    y[7] &= 0x7fffffffu;
    return ~strict_less(y, K_P) | strict_small_y(w);
}

}  // namespace c25519
