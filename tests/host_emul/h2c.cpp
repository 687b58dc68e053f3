// tests/host_emul/h2c.cpp -- TEST INFRASTRUCTURE.  The hashing calls' lane functions (curve25519_amd/csrc/h2c25519.cuh) driven on the
// CPU the way engine_h2c.hip drives them per lane: h2c_make_tail once per call as the host does it, then h2c_expand_lane,
// h2c_map_lane, h2c_to_curve_lane<2 / 1>, h2c_to_group_lane and h2c_to_scalar_lane per element, and the 48-byte reduction on its own
// for the property tests.  Built into its own library by tests/test_host_emul_h2c.py through tests/host_emul/build.py's open_lib.
// Not part of the product.
#include "emul.cpp"
#include "h2c25519.cuh"

extern "C" {

void emul_h2c_expand(unsigned char* out, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len,
                     size_t len_in_bytes, size_t n)
{
    H2cTail t;
    h2c_make_tail(t, msg_size, dst, dst_len, len_in_bytes);
    for (size_t i = 0; i < n; i++) h2c_expand_lane(out + i * len_in_bytes, msg + i * msg_size, t);
}

void emul_h2c_map(unsigned char* p, const unsigned char* u, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 uw[8], out[8];
        rd32(uw, u, i);
        h2c_map_lane(out, uw);
        wr32(p, i, out);
    }
}

// call: 0 HashToCurve, 1 EncodeToCurve, 2 HashToGroup, 3 HashToScalar
void emul_h2c_call(int call, unsigned char* p, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len, size_t n)
{
    H2cTail t;
    h2c_make_tail(t, msg_size, dst, dst_len, call == 0 ? 96 : call == 1 ? 48 : 64);
    for (size_t i = 0; i < n; i++) {
        u32 out[8];
        const uint8_t* m = msg + i * msg_size;
        switch (call) {
        case 0: h2c_to_curve_lane<2>(out, m, t); break;
        case 1: h2c_to_curve_lane<1>(out, m, t); break;
        case 2: h2c_to_group_lane(out, m, t); break;
        default: h2c_to_scalar_lane(out, m, t); break;
        }
        wr32(p, i, out);
    }
}

// 48 bytes big-endian -> the canonical 32 bytes of the value mod p
void emul_h2c_fe_from_be48(unsigned char* out, const unsigned char* in, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u64 d[6];
        for (int k = 0; k < 6; k++) {
            d[k] = 0;
            for (int j = 0; j < 8; j++) d[k] = (d[k] << 8) | in[48 * i + 8 * k + j];
        }
        fe r;
        u32 w[8];
        h2c_fe_from_be48(r, d);
        fe_to_words(w, r);
        wr32(out, i, w);
    }
}

}  // extern "C"
