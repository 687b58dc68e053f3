// tests/host_emul/verify_zip215.cpp -- TEST INFRASTRUCTURE.  The ZIP-215 verification (ed_zip215_decode, the cofactored walks, the
// Zip215 branches of the per-wave code and the cofactored reference-order fallback) compiled for the host against the C model of the
// gfx950 primitives, on top of everything tests/host_emul/emul.cpp drives (this file includes it):
//   emul_zip215_decode   ed_zip215_decode on raw 32-byte strings: canonical (x, y) and whether there is a square root;
//   emul_zip215_lane     the chain k_ed25519_verify_fast_scalars_zip215 (scalars times 8) -> _points_zip215 -> the plain walk, then
//                        k_ed25519_verify_slow_zip215 for the listed elements, one element at a time, with the kernels' own flag
//                        decisions (zip215_pair_flags, strict_key_flags: coop_ops.cuh);
//   emul_zip215_quad     k_ed25519_verify_quad_prep_zip215 -> _quad_walk_zip215: 16 elements per wave of lock-step lanes;
//   emul_zip215_waves    k_ed25519_verify_one_per_group_zip215: coop::verify_three_waves<false, true> as 192 lock-step lanes;
//   emul_zip215_plain_strict   the plain and the strict lane chains' verdicts, for the property test on honest signatures.
// listed[i] = 1 where the cofactored reference order decided the element, rejected[i] = 1 where it got verdict 0 without a walk.
// Built into its own library by tests/test_host_emul_verify_zip215.py through tests/host_emul/build.py's build_lib.
// Not part of the product.
#include "emul.cpp"

namespace {

int zip215_slow(const unsigned char* sig, const unsigned char* pk, const unsigned char* msg, size_t len, size_t i, std::vector<u32>& q)
{
    u32 pkw[8], Rw[8], Sw[8];
    rd32(pkw, pk, i);
    rd32(Rw, sig, 2 * i);
    rd32(Sw, sig, 2 * i + 1);
    return ed_verify_zip215_reference_order(pkw, Rw, Sw, msg + len * i, len, q.data(), tables() + (size_t)REF_TBL_OFFSET);
}

}  // namespace

extern "C" {

// xy: n x 64 bytes (canonical x, then canonical y mod p); ok[i] = 1 if the string decodes
void emul_zip215_decode(unsigned char* xy, int* ok, const unsigned char* enc, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 w[8], xw[8], yw[8];
        rd32(w, enc, i);
        fe X, Y;
        ok[i] = ed_zip215_decode(X, Y, w, 0u) ? 1 : 0;
        fe_to_words(xw, X);
        fe_to_words(yw, Y);
        wr32(xy, 2 * i, xw);
        wr32(xy, 2 * i + 1, yw);
    }
}

void emul_zip215_lane(int* verdict, int* listed, int* rejected, const unsigned char* sig, const unsigned char* pk, const unsigned char* msg,
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
        // scalars: rule 1 (verify_scalars_lane_zip215)
        const u32 lat_ok = ed_verify_zip215_scalars(cols, rho, tau, tau_neg, pkw, Rw, Sw, msg + len * i, len, cap, true);
        u32 f = (lat_ok & FLAG_FITS) | (tau_neg & FLAG_TAU_NEG) | zip215_pair_flags(Sw);
        // points: rules 2 and 3 (k_ed25519_verify_fast_points_zip215)
        fe QX, QY, RX, RY;
        const u32 q_ok = ed_zip215_decode(QX, QY, pkw, ~tau_neg);
        const u32 r_ok = ed_zip215_decode(RX, RY, Rw, 0xffffffffu);
        if (r_ok) f |= FLAG_R_OK;
        const u32 add = strict_key_flags(f, q_ok);
        f |= add;
        rejected[i] = (add & FLAG_REJECT) ? 1 : 0;
        listed[i] = (add & FLAG_SLOW) && !(add & FLAG_REJECT) ? 1 : 0;
        verdict[i] = 7;                                               // sentinel: an element nobody writes shows up
        if (add & FLAG_REJECT) { verdict[i] = 0; continue; }          // written by the key lane
        if (listed[i]) { verdict[i] = zip215_slow(sig, pk, msg, len, i, q); continue; }
        wtable_build(q.data(), QX, QY);
        wtable_build(q.data() + WTABLE_WORDS, RX, RY);
        const int top = walk_top_digit(tau, rho);
        const WalkScalars sc{ cols, tau, rho, 1, 0 };
        const u32 neutral = ge_walk_is_neutral(sc, q.data(), q.data() + WTABLE_WORDS, tbl, top < 8 ? 8 : top);
        verdict[i] = (neutral & f & FLAG_R_OK) ? 1 : 0;
    }
}

void emul_zip215_quad(int* verdict, int* listed, int* rejected, const unsigned char* sig, const unsigned char* pk, const unsigned char* msg,
                      size_t len, size_t n, int lat_cap_bits)
{
    std::lock_guard<std::mutex> lk(g_coop_mu);
    const u32* tbl = tables() + (size_t)SC_TBL_OFFSET;
    const int cap = lat_cap_bits > 0 ? lat_cap_bits : LAT_CAP_BITS;
    constexpr int G = quad::ELEMS_PER_WAVE;
    std::vector<u32> tabs((size_t)G * 2 * WTABLE_WORDS), cols((size_t)SIGMA_WORDS * G), rho(5 * G), tau(5 * G);
    std::vector<u32> q(QTABLE_LIMB_WORDS);
    for (size_t base = 0; base < n; base += G) {
        const int m = (int)std::min<size_t>(G, n - base);
        int wave_top = 0;
        u32 walks[G] = {}, flip[G] = {};
        for (int j = 0; j < m; j++) {
            const size_t i = base + j;
            u32 pkw[8], Rw[8], Sw[8], c[SIGMA_WORDS], rh[5], ta[5], tau_neg;
            rd32(pkw, pk, i);
            rd32(Rw, sig, 2 * i);
            rd32(Sw, sig, 2 * i + 1);
            const u32 lat_ok = ed_verify_zip215_scalars(c, rh, ta, tau_neg, pkw, Rw, Sw, msg + len * i, len, cap, false);
            const u32 f = (lat_ok & FLAG_FITS) | zip215_pair_flags(Sw);
            fe QX, QY, RX, RY;
            const u32 q_ok = ed_zip215_decode(QX, QY, pkw, 0xffffffffu);       // as k_ed25519_verify_quad_prep_zip215
            const u32 r_ok = ed_zip215_decode(RX, RY, Rw, 0xffffffffu);
            flip[j] = tau_neg;
            // k_ed25519_verify_quad_walk_zip215's decisions
            const bool rej = (f & FLAG_REJECT) || !q_ok || !r_ok;
            rejected[i] = rej ? 1 : 0;
            walks[j] = !rej && (f & FLAG_FITS);
            listed[i] = (!rej && !walks[j]) ? 1 : 0;
            verdict[i] = 7;
            if (rej) verdict[i] = 0;
            if (listed[i]) verdict[i] = zip215_slow(sig, pk, msg, len, i, q);
            if (!walks[j]) continue;
            wtable_build(tabs.data() + (size_t)j * 2 * WTABLE_WORDS, QX, QY);
            wtable_build(tabs.data() + (size_t)j * 2 * WTABLE_WORDS + WTABLE_WORDS, RX, RY);
            for (int w = 0; w < SIGMA_WORDS; w++) cols[(size_t)w * G + j] = c[w];
            for (int w = 0; w < 5; w++) { rho[(size_t)w * G + j] = rh[w]; tau[(size_t)w * G + j] = ta[w]; }
            wave_top = std::max(wave_top, walk_top_digit(ta, rh));
        }
        if (wave_top < 8) wave_top = 8;
        emul_coop::run_block(64, [&] {
            const int j = (int)(threadIdx.x >> 2);
            if (j >= m || !walks[j]) return;
            const quad::Roles R = quad::roles();
            const WalkScalars sc{ cols.data(), tau.data(), rho.data(), (size_t)G, (size_t)j };
            const u32* tq = tabs.data() + (size_t)j * 2 * WTABLE_WORDS;
            const u32 neutral = quad::walk_is_neutral<true>(sc, tq, tq + WTABLE_WORDS, tbl, wave_top, R, flip[j]);
            if (R.is0) verdict[base + j] = neutral ? 1 : 0;
        });
    }
}

void emul_zip215_waves(int* verdict, int* listed, int* rejected, const unsigned char* sig, const unsigned char* pk, const unsigned char* msg,
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
                coop::verify_three_waves<false, true>(lds.data(), park.data(), hand.data(), fs, verdict, sig, pk, msgs, n, e, tables());
            });
        }
    }
    for (size_t e = 0; e < n; e++) {
        rejected[e] = (flags[e] & FLAG_REJECT) ? 1 : 0;
        listed[e] = (flags[e] & FLAG_SLOW) ? 1 : 0;
    }
    for (u32 k = 0; k < counters[0]; k++) verdict[slow_list[k]] = zip215_slow(sig, pk, msg, len, slow_list[k], q);   // k_ed25519_verify_slow_zip215
}

// the plain lane chain (with its reference-order kernel) and the strict one, element by element
void emul_zip215_plain_strict(int* plain, int* strict, const unsigned char* sig, const unsigned char* pk, const unsigned char* msg,
                              size_t len, size_t n)
{
    std::vector<int> need(n);
    emul_ed25519_verify_fast(plain, need.data(), sig, pk, msg, len, n);
    std::vector<u32> q(QTABLE_LIMB_WORDS);
    for (size_t i = 0; i < n; i++) {
        u32 pkw[8], Rw[8], Sw[8], enc[8];
        rd32(pkw, pk, i);
        rd32(Rw, sig, 2 * i);
        rd32(Sw, sig, 2 * i + 1);
        if (need[i]) plain[i] = ed_verify_reference_order(pkw, Rw, Sw, msg + len * i, len, q.data(), tables() + (size_t)REF_TBL_OFFSET, enc);
        rd32(Sw, sig, 2 * i + 1);
        fe X, Y;
        const u32 key_ok = ed_verify_fast_decode(X, Y, pkw, 0u, 0u) & ~strict_reject_key(pkw);
        strict[i] = (key_ok && !strict_reject_pair(Rw, Sw)) ? plain[i] : 0;
    }
}

}  // extern "C"
