// tests/host_emul/verify_strict.cpp -- TEST INFRASTRUCTURE.  The strict verification (curve25519_amd/csrc/strict25519.cuh and the
// Strict branches of the lattice path) compiled for the host against the C model of the gfx950 primitives, on top of everything
// tests/host_emul/emul.cpp drives (this file includes it, so the library is one translation unit with its tables and scheduler):
//   emul_strict_predicates  the four predicates of strict25519.cuh on raw 32-byte values;
//   emul_strict_lane        the chain of k_ed25519_verify_fast_scalars_strict -> _points_strict -> k_ed25519_verify_fast_walk, then
//                           k_ed25519_verify_slow for the listed elements, one element at a time, with the kernels' own flag
//                           decisions (strict_pair_flags, strict_key_flags: coop_ops.cuh);
//   emul_strict_key         coop::strict_key_ok, the key check of k_ed25519_verify_check_strict_mask, by 64 lock-step lanes;
//   emul_strict_waves       k_ed25519_verify_one_per_group_strict: coop::verify_three_waves<true> as 192 lock-step lanes, then the
//                           reference order for the listed elements.
// Built into its own library by tests/test_host_emul_verify_strict.py through tests/host_emul/build.py's build_lib.
// Not part of the product.
#include "emul.cpp"
#include "strict25519.cuh"

extern "C" {

// out[4 i + 0] = v_i < L, [1] = strict_small_y(v_i), [2] = strict_reject_key(v_i), [3] = strict_reject_pair(R = v_i, S = v_i),
// each 1 or 0
void emul_strict_predicates(int* out, const unsigned char* v, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        rd32(w, v, i);
        out[4 * i + 0] = strict_less(w, K_L) ? 1 : 0;
        out[4 * i + 1] = strict_small_y(w) ? 1 : 0;
        out[4 * i + 2] = strict_reject_key(w) ? 1 : 0;
        out[4 * i + 3] = strict_reject_pair(w, w) ? 1 : 0;
    }
}

// listed[i] = 1 where the element went to the reference-order kernel, rejected[i] = 1 where it got FLAG_REJECT
void emul_strict_lane(int* verdict, int* listed, int* rejected, const unsigned char* sig, const unsigned char* pk, const unsigned char* msg,
                      size_t len, size_t n, int lat_cap_bits)
{
    const u32* tbl = tables() + (size_t)SC_TBL_OFFSET;
    std::vector<u32> q(2 * WTABLE_WORDS > QTABLE_LIMB_WORDS ? 2 * WTABLE_WORDS : QTABLE_LIMB_WORDS);
    const int cap = lat_cap_bits > 0 ? lat_cap_bits : LAT_CAP_BITS;
    for (size_t i = 0; i < n; i++) {
        u32 pkw[8], Rw[8], Sw[8], cols[SIGMA_WORDS], rho[5], tau[5], tau_neg;
        rd32(pkw, pk, i);
        rd32(Rw, sig, 2 * i);
        rd32(Sw, sig, 2 * i + 1);
        // scalars: rules 1 and 5 (verify_scalars_lane<true>)
        const u32 lat_ok = ed_verify_fast_scalars(cols, rho, tau, tau_neg, pkw, Rw, Sw, msg + len * i, len, cap);
        u32 f = (lat_ok & FLAG_FITS) | (tau_neg & FLAG_TAU_NEG) | strict_pair_flags(Rw, Sw);
        // points: the key lane applies rules 2-4 (verify_fast_points<true>), the R lane sets FLAG_R_OK
        fe QX, QY, RX, RY;
        const u32 q_ok = ed_verify_fast_decode(QX, QY, pkw, 0u, tau_neg) & ~strict_reject_key(pkw);
        const u32 r_ok = ed_verify_fast_decode(RX, RY, Rw, 0xffffffffu, tau_neg);
        if (r_ok) f |= FLAG_R_OK;
        const u32 add = strict_key_flags(f, q_ok);
        f |= add;
        rejected[i] = (add & FLAG_REJECT) ? 1 : 0;
        listed[i] = (add & FLAG_SLOW) && !(add & FLAG_REJECT) ? 1 : 0;
        verdict[i] = 7;
        if (add & FLAG_REJECT) { verdict[i] = 0; continue; }          // written by the key lane
        if (listed[i]) {                                              // k_ed25519_verify_slow
            u32 enc[8];
            verdict[i] = ed_verify_reference_order(pkw, Rw, Sw, msg + len * i, len, q.data(), tables() + (size_t)REF_TBL_OFFSET, enc);
            continue;
        }
        if (f & FLAG_SLOW) continue;                                  // the plain walk's test: skipped elements keep their verdict
        wtable_build(q.data(), QX, QY);
        wtable_build(q.data() + WTABLE_WORDS, RX, RY);
        const int top = walk_top_digit(tau, rho);
        const WalkScalars sc{ cols, tau, rho, 1, 0 };
        const u32 neutral = ge_walk_is_neutral(sc, q.data(), q.data() + WTABLE_WORDS, tbl, top < 8 ? 8 : top);
        verdict[i] = (neutral & f & FLAG_R_OK) ? 1 : 0;
    }
}

// coop::strict_key_ok (k_ed25519_verify_check_strict_mask's first wave) on n keys, 64 lock-step lanes each: ok[i] = 1 if key i keeps
// rules 2-4; every lane must agree (else ok[i] = 2)
void emul_strict_key(int* ok, const unsigned char* pk, size_t n)
{
    std::lock_guard<std::mutex> lk(g_coop_mu);
    std::vector<u32> lds(coop::LDS_WORDS);
    for (size_t i = 0; i < n; i++) {
        u32 w[8], votes[64];
        rd32(w, pk, i);
        emul_coop::run_block(64, [&] { votes[threadIdx.x] = coop::strict_key_ok(lds.data(), coop::make_lane(threadIdx.x), w); });
        ok[i] = votes[0] ? 1 : 0;
        for (int l = 1; l < 64; l++)
            if (votes[l] != votes[0]) ok[i] = 2;
    }
}

// sentinel: verdicts start at 7, so an element the kernel forgets to write shows up
void emul_strict_waves(int* verdict, int* listed, int* rejected, const unsigned char* sig, const unsigned char* pk, const unsigned char* msg,
                       size_t len, size_t n, int lat_cap_bits)
{
    std::vector<u32> lds(coop::V3_LDS_WORDS), park(40), hand(4), q(QTABLE_LIMB_WORDS);
    std::vector<u32> sigma((size_t)SIGMA_WORDS * n), rho(5 * n), tau(5 * n), flags(n), slow_list(n), counters(4, 0);
    FastScratch fs{};
    fs.sigma = sigma.data(); fs.rho = rho.data(); fs.tau = tau.data(); fs.flags = flags.data();
    fs.slow_list = slow_list.data(); fs.slow_count = counters.data();
    fs.lat_cap_bits = lat_cap_bits > 0 ? lat_cap_bits : LAT_CAP_BITS;
    const Msgs msgs{ msg, len, nullptr };
    {
        std::lock_guard<std::mutex> lk(g_coop_mu);
        for (size_t e = 0; e < n; e++) {
            verdict[e] = 7;
            emul_coop::run_block(192, [&] {
                coop::verify_three_waves<true>(lds.data(), park.data(), hand.data(), fs, verdict, sig, pk, msgs, n, e, tables());
            });
        }
    }
    for (size_t e = 0; e < n; e++) {
        rejected[e] = (flags[e] & FLAG_REJECT) ? 1 : 0;
        listed[e] = (flags[e] & FLAG_SLOW) ? 1 : 0;
    }
    for (u32 k = 0; k < counters[0]; k++) {                          // k_ed25519_verify_slow
        const size_t i = slow_list[k];
        u32 pkw[8], Rw[8], Sw[8], enc[8];
        rd32(pkw, pk, i);
        rd32(Rw, sig, 2 * i);
        rd32(Sw, sig, 2 * i + 1);
        verdict[i] = ed_verify_reference_order(pkw, Rw, Sw, msg + len * i, len, q.data(), tables() + (size_t)REF_TBL_OFFSET, enc);
    }
}

}  // extern "C"
