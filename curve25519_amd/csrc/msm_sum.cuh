// curve25519_amd/csrc/msm_sum.cuh -- what ONE lane does for the multiscalar multiplications (include/curve25519_amd.h states their
// rules):
//   ed25519_MultiScalarMult[_vartime]_*        Q_g = sum_i [s_i mod L] P_i over the m rows of group g, Edwards points (ZIP-215 decoding)
//   ristretto255_MultiScalarMult[_vartime]_*   the same on ristretto255 (RFC 9496 DECODE / ENCODE)
// engine_msm.hip wraps these in its kernels; tests/host_emul/msm.cpp drives the same functions on the CPU.
//
// Two paths, one contract (the same bytes: s_i is read mod L in both, so a torsion part of an Edwards point is multiplied alike):
//   * the constant-time path (the plain calls, and the _vartime calls below MSM_BUCKET_MIN).  Rows: one lane per row does sc_mod,
//     decodes, runs ed_group.cuh's walk -- table in registers, rows selected by masks -- and leaves the EXTENDED point (the walk's last
//     addition does not form T: it is re-formed as (X Z, Y Z, Z^2, X Y), as ristretto255.cuh's encoding does) and the decode flag.
//     Sum: one lane adds at most MSM_SUM_CHUNK consecutive points of one group by the complete addition and ANDs their flags; passes
//     repeat until a group has one point.  Finish: the group's encoding.  Nothing but data depends on a scalar: which rows a lane
//     reads is a function of m alone.
//   * the bucket path (the _vartime calls from MSM_BUCKET_MIN): msm25519.cuh's stages per group.  The packed row holds P itself
//     (msm_point_row stores -P for the batch equation; here nothing is negated anywhere), the scalar is sc_mod then msm_bias, and the
//     tail is Horner over the wa windows a scalar below L has, then the encoding.  Bucket addresses depend on the digits.
#pragma once
#include "msm25519.cuh"
#include "ristretto255.cuh"

namespace c25519 {

constexpr int MSM_SUM_CHUNK = 64;                           // points one lane adds in sequence
constexpr int MSM_GROUP_EDWARDS = 0, MSM_GROUP_R255 = 1;    // the kernels' group parameter
constexpr int MSM_WALK_WINDOW = 2;                          // the group calls' built-in width (engine_group.hip, engine_ristretto.hip)

// (X, Y) affine and reduced, all-ones iff the 32 bytes decode under the group's rule
template <int G>
C25519_DEV u32 msm_sum_decode(fe& X, fe& Y, const u32 (&pw)[8])
{
    if constexpr (G == MSM_GROUP_EDWARDS) return ed_zip215_decode(X, Y, pw, 0u);
    else return rist_decode(X, Y, pw, 0u);
}

// s mod L for all 256 bits of s
C25519_DEV void msm_sum_scalar(u32 (&e)[8], const u32 (&sw)[8])
{
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = sw[i];
    sc_mod(e);
}

// the rows stage for one row: S = [s mod L] P extended, returns all-ones iff the point bytes decode (a row that does not decode
// walks too: its group's output is masked)
template <int G, int W>
C25519_DEV u32 msm_sum_row_lane(ge_ext& S, const u32 (&sw)[8], const u32 (&pw)[8])
{
    fe X, Y;
    const u32 ok = msm_sum_decode<G>(X, Y, pw);
    u32 e[8];
    msm_sum_scalar(e, sw);
    ed_group_walk<W>(S, X, Y, e);
    fe x, y, z;
    fe_mul(S.T, S.X, S.Y);
    fe_mul(x, S.X, S.Z);
    fe_mul(y, S.Y, S.Z);
    fe_sqr(z, S.Z);
    S.X = x;
    S.Y = y;
    S.Z = z;
    return ok;
}

// the sum stage for one chunk: S = the sum of the `count` >= 1 points from `first` on (40 words each), returns the AND of their flags
C25519_DEV u32 msm_sum_chunk_lane(ge_ext& S, const u32* __restrict__ pts, const u32* __restrict__ flags, size_t first, u32 count)
{
    msm_load_ext(S, pts + first * MSM_EXT_WORDS);
    u32 ok = flags[first];
#pragma unroll 1
    for (u32 i = 1; i < count; i++) {
        ge_ext t;
        msm_load_ext(t, pts + (first + i) * MSM_EXT_WORDS);
        msm_ext_add(S, t);
        ok &= flags[first + i];
    }
    return ok;
}

// the group's encoding of an extended point by the lane's own inversion (the constant-time path's Edwards finish goes through the
// shared inversion instead: FinishGroupPoint)
template <int G>
C25519_DEV void msm_sum_encode(u32 (&out)[8], const ge_ext& S)
{
    if constexpr (G == MSM_GROUP_EDWARDS) msm_encode(out, S);
    else rist_encode<true>(out, S);
}

// ---- the bucket path ----

// the packed 128-byte row of P (Y+X | Y-X | 2dXY), 24 words used.  Returns all-ones iff the string decodes.
template <int G>
C25519_DEV u32 msm_sum_point_row(u32 (&row)[24], const u32 (&enc)[8])
{
    fe X, Y, t;
    const u32 ok = msm_sum_decode<G>(X, Y, enc);
    u32 w[8];
    fe_add(t, Y, X);  fe_carry32(t, t);  fe_to_words(w, t);
#pragma unroll
    for (int j = 0; j < 8; j++) row[j] = w[j];
    fe_sub(t, Y, X);  fe_carry32(t, t);  fe_to_words(w, t);
#pragma unroll
    for (int j = 0; j < 8; j++) row[8 + j] = w[j];
    fe_mul(t, X, Y);
    fe_mul(t, t, fe_const(K_2D));
    fe_to_words(w, t);
#pragma unroll
    for (int j = 0; j < 8; j++) row[16 + j] = w[j];
    return ok;
}

// s mod L, BIASED for width c
C25519_DEV void msm_sum_biased_scalar(u32 (&k)[8], const u32 (&sw)[8], int c)
{
    msm_sum_scalar(k, sw);
    msm_bias(k, c, msm_windows_a(c));
}

// T = sum_w 2^(c w) Window_w over the wa windows
C25519_DEV void msm_sum_horner(ge_ext& T, const u32* __restrict__ windows, const MsmShape& sh)
{
    ge_ext t;
    msm_load_ext(T, windows + (size_t)(sh.wa - 1) * MSM_EXT_WORDS);
#pragma unroll 1
    for (int w = sh.wa - 2; w >= 0; w--) {
#pragma unroll 1
        for (int j = 0; j < sh.c - 1; j++) ge_double<false>(T);
        ge_double<true>(T);
        msm_load_ext(t, windows + (size_t)w * MSM_EXT_WORDS);
        msm_ext_add(T, t);
    }
}

}  // namespace c25519
