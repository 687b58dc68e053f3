// tests/host_emul/ristretto.cpp -- TEST INFRASTRUCTURE.  The ristretto255 calls' lane functions (curve25519_amd/csrc/ristretto255.cuh)
// driven on the CPU the way engine_ristretto.hip drives them per lane: rist_decode for IsValidPoint, rist_from_hash_lane,
// rist_scalarmult_lane<W>, rist_base_lane over the wide comb emul.cpp builds, rist_add_lane, and decode / encode / map on their own for
// the property tests.  Built into its own library by tests/test_host_emul_ristretto.py through tests/host_emul/build.py's open_lib.
// Not part of the product.
#include "emul.cpp"
#include "ristretto255.cuh"

extern "C" {

void emul_rist_is_valid(int* ok, const unsigned char* point, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 pw[8];
        rd32(pw, point, i);
        fe X, Y;
        ok[i] = (int)(rist_decode(X, Y, pw, 0u) & 1u);
    }
}

void emul_rist_from_hash(unsigned char* p, const unsigned char* hash, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 lo[8], hi[8], out[8];
        rd32(lo, hash, 2 * i);
        rd32(hi, hash, 2 * i + 1);
        rist_from_hash_lane(out, lo, hi);
        wr32(p, i, out);
    }
}

void emul_rist_scalarmult(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t n, int w)
{
    for (size_t i = 0; i < n; i++) {
        u32 sw[8], pw[8], out[8];
        rd32(sw, scalar, i);
        rd32(pw, point, i);
        const u32 accept = w == 4 ? rist_scalarmult_lane<4>(out, sw, pw) : w == 3 ? rist_scalarmult_lane<3>(out, sw, pw)
                                                                                  : rist_scalarmult_lane<2>(out, sw, pw);
        ok[i] = (int)(accept & 1u);
        wr32(q, i, out);
    }
}

void emul_rist_base(unsigned char* q, const unsigned char* scalar, size_t n)
{
    const u32* wide = wide_tables();
    for (size_t i = 0; i < n; i++) {
        u32 sw[8], out[8];
        rd32(sw, scalar, i);
        unsigned short cols[WB_COLS];
        rist_base_lane(out, sw, wide, cols, 1);
        wr32(q, i, out);
    }
}

void emul_rist_add(unsigned char* r, int* ok, const unsigned char* p, const unsigned char* q, size_t n, int sub)
{
    for (size_t i = 0; i < n; i++) {
        u32 pw[8], qw[8], out[8];
        rd32(pw, p, i);
        rd32(qw, q, i);
        const u32 accept = rist_add_lane(out, pw, qw, sub ? 0xffffffffu : 0u);
        ok[i] = (int)(accept & 1u);
        wr32(r, i, out);
    }
}

// DECODE then ENCODE of the decoded point as it stands (x, y, 1, x y): enc is the input again where ok; xy: the canonical x and y
void emul_rist_decode_encode(unsigned char* enc, unsigned char* xy, int* ok, const unsigned char* point, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 pw[8], out[8], xw[8], yw[8];
        rd32(pw, point, i);
        ge_ext S;
        ok[i] = (int)(rist_decode(S.X, S.Y, pw, 0u) & 1u);
        fe_set_u32(S.Z, 1);
        fe_mul(S.T, S.X, S.Y);
        rist_encode<true>(out, S);
        wr32(enc, i, out);
        fe_to_words(xw, S.X);
        fe_to_words(yw, S.Y);
        wr32(xy, 2 * i, xw);
        wr32(xy, 2 * i + 1, yw);
    }
}

// ENCODE of the affine point (x, y) given as 2 x 32 canonical bytes, scaled by the projective factor z (32 bytes): with T
// (with_t != 0: rist_encode<true> on (x z, y z, z, x y z)) or re-formed (rist_encode<false>)
void emul_rist_encode_affine(unsigned char* enc, const unsigned char* xy, const unsigned char* z, size_t n, int with_t)
{
    for (size_t i = 0; i < n; i++) {
        u32 xw[8], yw[8], zw[8], out[8];
        rd32(xw, xy, 2 * i);
        rd32(yw, xy, 2 * i + 1);
        rd32(zw, z, i);
        fe x, y;
        ge_ext S;
        fe_from_words(x, xw);
        fe_from_words(y, yw);
        fe_from_words(S.Z, zw);
        fe_mul(S.X, x, S.Z);
        fe_mul(S.Y, y, S.Z);
        fe_mul(S.T, x, S.Y);
        if (with_t) rist_encode<true>(out, S);
        else rist_encode<false>(out, S);
        wr32(enc, i, out);
    }
}

}  // extern "C"
