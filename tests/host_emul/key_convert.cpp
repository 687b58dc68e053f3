// tests/host_emul/key_convert.cpp -- TEST INFRASTRUCTURE.  The key calls' lane functions (curve25519_amd/csrc/ed_keys.cuh) driven on
// the CPU the way engine_keys.hip drives them per lane: k_ed25519_key_classify's ed_key_classify, k_ed25519_key_to_x25519's
// ed_key_to_x25519_lane with FinishKeyX25519 behind a plain fe_invert (the shared inversion's answer, 0 for a zero denominator),
// k_ed25519_private_to_x25519's ed_key_private_to_x25519, and the walk's pieces on their own for the property tests.  Built into
// its own library by tests/test_host_emul_key_convert.py through tests/host_emul/build.py's open_lib.  Not part of the product.
#define EMUL_COOP_WAVE_IMPL 1
#include "coop_wave.h"
#include "ed_keys.cuh"

#include <thread>
#include <vector>

using namespace c25519;

namespace c25519 { unsigned long long emul_mad_overflows = 0, emul_mad_count = 0; LatCounters emul_lat_counters = { 0, 0, 0 }; }
thread_local EmulWave* emul_wave = nullptr;
thread_local emul_dim3 emul_tid = { 0, 0, 0 };

namespace {

void rd32(u32 (&w)[8], const unsigned char* p, size_t i) { memcpy(w, p + 32 * i, 32); }

}  // namespace

extern "C" {

unsigned long long emul_mad_overflow_count(void) { return emul_mad_overflows; }

// the two generated digit masks of L, 8 words each
void emul_key_naf_masks(unsigned* nz, unsigned* neg)
{
    for (int i = 0; i < 8; i++) { nz[i] = K_L_NAF_NZ[i]; neg[i] = K_L_NAF_NEG[i]; }
}

void emul_key_classify(unsigned* flags, const unsigned char* pk, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        rd32(w, pk, i);
        fe X, Y;
        flags[i] = ed_key_classify(X, Y, w);
    }
}

// the scratch of one element at a time (struct-of-arrays with n = 1), as the kernel and the shared inversion's finish use it
void emul_key_to_x25519(unsigned char* xpk, int* ok, const unsigned char* pk, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 w[8], num_words[10], ok_word;
        rd32(w, pk, i);
        fe num, den, zinv;
        ok_word = ed_key_to_x25519_lane(num, den, w);
        ok[i] = ok_word ? 1 : 0;
        soa_store_fe(num_words, 1, 0, num);
        fe_invert(zinv, den);
        const FinishKeyX25519 fin{ num_words, &ok_word, xpk + 32 * i, 1 };
        fin.emit(0, zinv);
    }
}

void emul_key_private_to_x25519(unsigned char* xsk, const unsigned char* priv, size_t n)
{
    for (size_t i = 0; i < n; i++) ed_key_private_to_x25519(xsk, priv, i);
}

// for bytes that decode: small[i] = the SMALL_ORDER predicate on the bytes, times8[i] = ([8]A == O) by three doublings of the lane's
// own point arithmetic and the walk's neutral test, walk_xy = the affine (x, y) of [L]A (n x 64 bytes, canonical);
// decodes[i] = 0 and the rest untouched where they do not
void emul_key_order_parts(int* decodes, int* small, int* times8, unsigned char* walk_xy, const unsigned char* pk, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 w[8], xw[8], yw[8];
        rd32(w, pk, i);
        fe X, Y;
        decodes[i] = ed_zip215_decode(X, Y, w, 0u) ? 1 : 0;
        if (!decodes[i]) continue;
        small[i] = strict_small_y(w) ? 1 : 0;
        ge_ext S;
        S.X = X; S.Y = Y;
        fe_set_u32(S.Z, 1);
        for (int j = 0; j < 3; j++) ge_double<false>(S);
        times8[i] = ge_is_neutral(S) ? 1 : 0;
        ed_key_walk_L(S, X, Y);
        ge_to_affine_words(xw, yw, S);
        memcpy(walk_xy + 64 * i, xw, 32);
        memcpy(walk_xy + 64 * i + 32, yw, 32);
    }
}

}  // extern "C"
