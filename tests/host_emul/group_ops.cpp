// tests/host_emul/group_ops.cpp -- TEST INFRASTRUCTURE.  The group calls' lane functions (curve25519_amd/csrc/ed_group.cuh) driven on
// the CPU the way engine_group.hip drives them per lane: k_ed25519_group_scalarmult<W>'s ed_group_scalarmult_lane and
// k_ed25519_group_add's ed_group_add_lane with FinishGroupPoint behind a plain fe_invert (the shared inversion's answer),
// k_ed25519_group_base's ed_group_base_lane over the wide comb emul.cpp builds, and the recoding on its own for the property tests.
// Built into its own library by tests/test_host_emul_group_ops.py through tests/host_emul/build.py's open_lib.  Not part of the
// product.
#include "emul.cpp"
#include "ed_group.cuh"

namespace {

// the scratch of one element at a time (struct-of-arrays with n = 1), as the kernels and the shared inversion's finish use it
void group_finish(unsigned char* out, const ge_ext& S, u32 ok_word)
{
    u32 xs[10], ys[10];
    soa_store_fe(xs, 1, 0, S.X);
    soa_store_fe(ys, 1, 0, S.Y);
    fe zinv;
    fe_invert(zinv, S.Z);
    const FinishGroupPoint fin{ xs, ys, &ok_word, out, 1 };
    fin.emit(0, zinv);
}

template <int W>
void group_digits(int* out, const u32 (&e)[8])
{
    u32 t[9];
    group_recode<W>(t, e);
    for (int i = GroupWindow<W>::DIGITS - 1; i >= 0; i--) out[i] = (int)group_next_field<W>(t) - GroupWindow<W>::ROWS;
}

}  // namespace

extern "C" {

// q, ok of ed25519_ScalarMult (clamp != 0) / ed25519_ScalarMult_noclamp at window width w
void emul_group_scalarmult(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t n, int w, int clamp)
{
    for (size_t i = 0; i < n; i++) {
        u32 sw[8], pw[8];
        rd32(sw, scalar, i);
        rd32(pw, point, i);
        ge_ext S;
        const u32 cm = clamp ? 0xffffffffu : 0u;
        const u32 accept = w == 4 ? ed_group_scalarmult_lane<4>(S, sw, pw, cm)
                         : w == 3 ? ed_group_scalarmult_lane<3>(S, sw, pw, cm) : ed_group_scalarmult_lane<2>(S, sw, pw, cm);
        ok[i] = accept ? 1 : 0;
        group_finish(q + 32 * i, S, accept);
    }
}

void emul_group_base(unsigned char* q, const unsigned char* scalar, size_t n, int clamp)
{
    const u32* wide = wide_tables();
    for (size_t i = 0; i < n; i++) {
        u32 sw[8], enc[8];
        rd32(sw, scalar, i);
        unsigned short cols[WB_COLS];
        ge_ext S;
        ed_group_base_lane(S, sw, clamp ? 0xffffffffu : 0u, wide, cols, 1);
        affine_pack_host(enc, S);
        wr32(q, i, enc);
    }
}

void emul_group_add(unsigned char* r, int* ok, const unsigned char* p, const unsigned char* q, size_t n, int sub)
{
    for (size_t i = 0; i < n; i++) {
        u32 pw[8], qw[8];
        rd32(pw, p, i);
        rd32(qw, q, i);
        ge_ext S;
        const u32 accept = ed_group_add_lane(S, pw, qw, sub ? 0xffffffffu : 0u);
        ok[i] = accept ? 1 : 0;
        group_finish(r + 32 * i, S, accept);
    }
}

// the signed digits of e (clamped or the low 255 bits), least significant first: 129 / 86 / 65 ints for w = 2 / 3 / 4
void emul_group_digits(int* out, const unsigned char* scalar, int w, int clamp)
{
    u32 sw[8], e[8];
    rd32(sw, scalar, 0);
    group_scalar(e, sw, clamp ? 0xffffffffu : 0u);
    if (w == 4) group_digits<4>(out, e);
    else if (w == 3) group_digits<3>(out, e);
    else group_digits<2>(out, e);
}

}  // extern "C"
