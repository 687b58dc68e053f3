// tests/host_emul/vrf.cpp -- TEST INFRASTRUCTURE.  The ECVRF calls' lane functions (curve25519_amd/csrc/vrf25519.cuh) driven on the
// CPU the way engine_vrf.hip drives them per lane: vrf_make_tail once per call as the host does it, then vrf_prove_lane,
// vrf_verify_lane and vrf_proof_to_hash_lane per element over the wide comb emul.cpp builds, and the recoding on its own for the
// property tests.  Built into its own library by tests/test_host_emul_vrf.py through tests/host_emul/build.py's open_lib.  Not part
// of the product.
#include "emul.cpp"
#include "vrf25519.cuh"

namespace {

// element i's 64-byte private key as vrf_prove_lane reads it (engine_vrf.hip: VrfKeyAt)
struct EmulKeyAt {
    const unsigned char* priv; size_t i;
    void seed(u32 (&w)[8]) const { rd32(w, priv, 2 * i); }
    void pk(u32 (&w)[8]) const { rd32(w, priv, 2 * i + 1); }
};

}  // namespace

extern "C" {

void emul_vrf_prove(unsigned char* proof, const unsigned char* priv, const unsigned char* alpha, size_t alpha_size, size_t n)
{
    const u32* wide = wide_tables();
    H2cTail t;
    vrf_make_tail(t, alpha_size);
    for (size_t i = 0; i < n; i++) {
        u32 pi[VRF_PROOF_WORDS];
        unsigned short cols[WB_COLS];
        vrf_prove_lane(pi, EmulKeyAt{ priv, i }, alpha + i * alpha_size, t, wide, cols, 1);
        memcpy(proof + 80 * i, pi, 80);
    }
}

void emul_vrf_verify(unsigned char* beta, int* ok, const unsigned char* pk, const unsigned char* proof, const unsigned char* alpha,
                     size_t alpha_size, size_t n)
{
    const u32* wide = wide_tables();
    H2cTail t;
    vrf_make_tail(t, alpha_size);
    for (size_t i = 0; i < n; i++) {
        u32 pkw[8], pi[VRF_PROOF_WORDS], b[VRF_BETA_WORDS];
        unsigned short cols[WB_COLS];
        rd32(pkw, pk, i);
        memcpy(pi, proof + 80 * i, 80);
        const u32 accept = vrf_verify_lane(b, pkw, pi, alpha + i * alpha_size, t, wide, cols, 1);
        memcpy(beta + 64 * i, b, 64);
        ok[i] = accept ? 1 : 0;
    }
}

void emul_vrf_proof_to_hash(unsigned char* beta, int* ok, const unsigned char* proof, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 pi[VRF_PROOF_WORDS], b[VRF_BETA_WORDS];
        memcpy(pi, proof + 80 * i, 80);
        const u32 accept = vrf_proof_to_hash_lane(b, pi);
        memcpy(beta + 64 * i, b, 64);
        ok[i] = accept ? 1 : 0;
    }
}

// the signed two-bit digits of e, least significant first: 129 ints (full != 0, e below 2^255) or 65 (e below 2^128)
void emul_vrf_digits(int* out, const unsigned char* scalar, int full)
{
    u32 e[8], t[9];
    rd32(e, scalar, 0);
    if (full) {
        vrf_recode<VRF_DIGITS_FULL>(t, e);
        for (int i = VRF_DIGITS_FULL - 1; i >= 0; i--) out[i] = (int)group_next_field<2>(t) - 2;
    } else {
        vrf_recode<VRF_DIGITS_C>(t, e);
        for (int i = VRF_DIGITS_C - 1; i >= 0; i--) out[i] = (int)group_next_field<2>(t) - 2;
    }
}

}  // extern "C"
