// tests/host_emul/scalar.cpp -- TEST INFRASTRUCTURE.  The scalar calls' lane functions (curve25519_amd/csrc/sc_invert.cuh) driven on
// the CPU the way engine_scalar.hip drives them per lane: sc_op_lane for the element-wise calls, sc_is_canonical, and
// sc_invert_lane<K> over ceil(n / K) lanes with the K = 16 kernel's LDS parking area as a plain array.  Built into its own library by
// tests/test_host_emul_scalar.py through tests/host_emul/build.py's open_lib.  Not part of the product.
#include "emul.cpp"
#include "sc_invert.cuh"

template <int K>
static void emul_scalar_invert_k(unsigned char* recip, int* ok, const unsigned char* s, size_t n)
{
    u32 park[sc_invert_parked<K>() * 8 + 1];
    for (size_t lane = 0; lane * K < n; lane++) sc_invert_lane<K>(recip, ok, s, n, lane, park, 1);
}

extern "C" {

// op: sc_invert.cuh's ScOp; b and c may be null where the operation does not read them; r may be a, b or c
void emul_scalar_op(int op, unsigned char* r, const unsigned char* a, const unsigned char* b, const unsigned char* c, size_t n)
{
    for (size_t i = 0; i < n; i++) sc_op_lane(op, r, a, b, c, i);
}

void emul_scalar_is_canonical(int* ok, const unsigned char* s, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        rd32(w, s, i);
        ok[i] = (int)sc_is_canonical(w);
    }
}

// k: 1, 2, 4, 8 or 16; returns 0 for any other
int emul_scalar_invert(unsigned char* recip, int* ok, const unsigned char* s, size_t n, int k)
{
    switch (k) {
    case 16: emul_scalar_invert_k<16>(recip, ok, s, n); break;
    case 8: emul_scalar_invert_k<8>(recip, ok, s, n); break;
    case 4: emul_scalar_invert_k<4>(recip, ok, s, n); break;
    case 2: emul_scalar_invert_k<2>(recip, ok, s, n); break;
    case 1: emul_scalar_invert_k<1>(recip, ok, s, n); break;
    default: return 0;
    }
    return k;
}

// sc_invert_words on its own: any 32-byte value, zero included (0 -> 0)
void emul_scalar_invert_words(unsigned char* out, const unsigned char* in, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 x[8], y[8];
        rd32(x, in, i);
        sc_invert_words(y, x);
        wr32(out, i, y);
    }
}

}  // extern "C"
