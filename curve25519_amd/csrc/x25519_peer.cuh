// curve25519_amd/csrc/x25519_peer.cuh -- X25519 against ONE peer key over a wide comb built for that key: what one lane does
// to prepare the peer's point, and what one lane does per secret.  engine_x25519.hip wraps these in its one-peer kernels;
// tests/host_emul/one_peer.cpp drives the same functions on the CPU.
//
// The identity.  The clamped scalar k is a multiple of 8, so k * P = (k >> 3) * (8 P), and Q = 8 P lies in the subgroup of
// prime order L whatever torsion component P carries.  x(k P) -- the ladder's output, curve25519_dh.c:111-150 -- is then the
// fixed-base walk of ge25519.cuh (ge_base_mult_wide) over a comb built for Q, with the scalar k >> 3 < 2^252 (wb_columns adds
// L when it is even, as it does for the base point: L * Q = O), finished as u = (Z + Y) / (Z - Y) exactly like
// curve25519_dh_CalculatePublicKey_fast (k_x25519_public_fast_mult).  For a P of small order Q is the neutral element, the
// walk ends at (0 : Z : Z), the denominator is zero and the shared inversion gives 0 -- the ladder's answer too.
//
// Eligibility.  The peer's u is read as the reference reads it: all 256 bits, bit 255 included, mod p (fe_from_words).
// Edwards y = (u - 1) / (u + 1); u = -1 has no image (and is a twist point: fe_invert(0) = 0 would give y = 0 and a bogus
// x = sqrt(-1)), so it is refused outright.  For every other u, ge_calc_x_checked's verdict is the curve's: a u on the
// quadratic twist has no x and goes to the ladder.  Either root x will do -- only x(k P) leaves, and x(k (-P)) = x(k P).
// The peer key is public: branching on its eligibility leaks nothing.  The secret only selects table rows, as it does in
// every fixed-base walk of the library.
#pragma once
#include "fe25519.cuh"
#include "ge25519.cuh"

namespace c25519 {

constexpr int PEER_Q_WORDS = 24;          // Q in affine precomputed form, canonical words: Y+X | Y-X | 2dT

// Q = 8 P for the peer u-coordinate `u` (32 bytes as little-endian words); returns all-ones when the comb may stand in for
// the ladder (u != -1 mod p and u on the curve), 0 otherwise (q is then meaningless)
C25519_DEV u32 x25519_peer_point(u32 (&q)[3][8], const u32 (&u)[8])
{
    fe U, one, num, den, inv, t;
    fe_from_words(U, u);
    fe_set_u32(one, 1);
    fe_sub(t, U, one);  fe_carry32(num, t);              // u - 1
    fe_add(t, U, one);  fe_carry32(den, t);              // u + 1
    u32 w[8], nz = 0;
    fe_to_words(w, den);
#pragma unroll
    for (int i = 0; i < 8; i++) nz |= w[i];
    fe_invert(inv, den);
    ge_ext P;
    fe_mul(P.Y, num, inv);                               // y = (u - 1) / (u + 1)
    const u32 on_curve = ge_calc_x_checked(P.X, P.Y, 0);
    fe_mul(P.T, P.X, P.Y);
    fe_set_u32(P.Z, 1);
    ge_double<false>(P);
    ge_double<false>(P);
    ge_double<false>(P);                                 // Q = 8 P: only X, Y, Z are read below
    fe zi, x, y, row[3];
    fe_invert(zi, P.Z);
    fe_mul(x, P.X, zi);
    fe_mul(y, P.Y, zi);
    fe_add(row[0], y, x);
    fe_sub(row[1], y, x);
    fe_mul(t, x, y);
    fe_mul(row[2], t, fe_const(K_2D));
#pragma unroll
    for (int f = 0; f < 3; f++) fe_to_words(q[f], row[f]);
    return (nz != 0 && on_curve) ? 0xffffffffu : 0u;
}

// Q back from its canonical words (reduced limbs, as table rows are read)
C25519_DEV void x25519_peer_pa(ge_pa& Q, const u32* q_words)
{
    u32 w[8];
#pragma unroll
    for (int f = 0; f < 3; f++) {
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = q_words[8 * f + j];
        fe_from_words(f == 0 ? Q.ypx : f == 1 ? Q.ymx : Q.t2d, w);
    }
}

// one secret against the peer: k = the CLAMPED scalar words, wide_peer = the WB_NT packed tables of Q's comb (ge_signed_comb_row_of
// of Q, laid out as k_gen_wide_table lays out the base point's), cols = this lane's parked columns `stride` apart.  The
// numerator and denominator of u = (Z + Y) / (Z - Y), for the shared inversion (FinishX25519).
template <typename ColT>
C25519_DEV void x25519_one_peer_lane(fe& num, fe& den, const u32 (&k)[8], const u32* __restrict__ wide_peer, ColT* cols, int stride)
{
    u32 k3[8];                                           // k >> 3: exact, the three low bits are clear
#pragma unroll
    for (int i = 0; i < 7; i++) k3[i] = (k[i] >> 3) | (k[i + 1] << 29);
    k3[7] = k[7] >> 3;
    wb_columns(cols, stride, k3);                        // k3 + L when even: Q has order L (or 1)
    ge_ext S;
    ge_base_mult_wide(S, wide_peer, cols, stride);
    fe t;
    fe_add(t, S.Z, S.Y);  fe_carry32(num, t);
    fe_sub(t, S.Z, S.Y);  fe_carry32(den, t);
}

}  // namespace c25519
