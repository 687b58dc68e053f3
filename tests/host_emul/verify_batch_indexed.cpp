// tests/host_emul/verify_batch_indexed.cpp -- TEST INFRASTRUCTURE.  The lane-level code of the ZIP-215 batch equation with coalesced
// keys (curve25519_amd/csrc/msm25519.cuh: msm_scalars_canonical, msm_key_fold and every stage the plain equation has) compiled for the
// host against the C model of the gfx950 primitives, on top of everything tests/host_emul/emul.cpp drives (this file includes it).
// What the k_ed25519_keyeq_* kernels of engine_batch_eq.hip do across lanes -- the per-key sums in LDS and memory, the counting sort
// with atomics, the reductions -- is done here by plain host loops:
//   emul_keyeq_fold   eight 64-bit word sums -> the key's scalar mod L, biased for width c (msm_key_fold), and whether it is non-zero;
//   emul_keyeq        the whole chain for one call: enc(T) as the hook returns it, and the result.
// Built into its own library by tests/test_host_emul_verify_batch_indexed.py through tests/host_emul/build.py's build_lib.
// Not part of the product.
#include "emul.cpp"
#include "msm25519.cuh"

extern "C" {

// scalar: 32 bytes, the BIASED total; returns 1 iff the total mod L is not zero
int emul_keyeq_fold(unsigned char* scalar, const unsigned long long* sums, int c)
{
    u64 sum[8];
    for (int j = 0; j < 8; j++) sum[j] = sums[j];
    u32 a[8];
    const u32 any = msm_key_fold(a, sum, c);
    wr32(scalar, 0, a);
    return any ? 1 : 0;
}

// point: 32 bytes, enc(T) over the elements that stay; returns the result of the call
int emul_keyeq(unsigned char* point, const unsigned char* keys, size_t K, const unsigned int* key_index, const unsigned char* sig,
               const unsigned char* msg, size_t len, size_t n, const unsigned char* seed, int c)
{
    const size_t N = K + n;
    const MsmShape sh = msm_shape(c);
    const int wa = sh.wa, wz = sh.wz, buckets = sh.buckets;
    u32 seedw[8];
    rd32(seedw, seed, 0);
    std::vector<u32> rows(N * MSM_ROW_WORDS, 0), sc(8 * N), flags(N, 0);
    bool reject = false;
    // points (k_ed25519_keyeq_points): a key that does not decode only gets its flag
    for (size_t j = 0; j < N; j++) {
        u32 w[8], row[24];
        if (j >= K) rd32(w, sig, 2 * (j - K)); else rd32(w, keys, j);
        if (!msm_point_row(row, w)) {
            flags[j] = 1;
            if (j >= K) reject = true;
        }
        memcpy(&rows[j * MSM_ROW_WORDS], row, sizeof row);
    }
    // scalars (k_ed25519_keyeq_scalars): the s_i leave as sums of 16-bit chunks, the a_i as eight word sums per key
    u64 chunk[16] = {};
    std::vector<u64> keysum(8 * K, 0);
    for (size_t i = 0; i < n; i++) {
        u32 pkw[8], Rw[8], Sw[8], a[8], z[8], s[8];
        const u32 idx = key_index[i];
        const bool in_range = idx < K;
        rd32(pkw, keys, in_range ? idx : 0);
        rd32(Rw, sig, 2 * i);
        rd32(Sw, sig, 2 * i + 1);
        const u32 s_ok = msm_scalars_canonical(a, z, s, pkw, Rw, Sw, msg + len * i, len, seedw, i, c);
        for (int j = 0; j < 8; j++) sc[j * N + K + i] = z[j];
        if (!s_ok || !in_range || flags[K + i] || flags[idx]) {
            flags[K + i] = 1;
            reject = true;
            continue;
        }
        for (int j = 0; j < 16; j++) chunk[j] += (s[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        for (int j = 0; j < 8; j++) keysum[8 * (size_t)idx + j] += a[j];
    }
    // fold (k_ed25519_keyeq_fold)
    for (size_t k = 0; k < K; k++) {
        u64 sum[8];
        u32 a[8];
        for (int j = 0; j < 8; j++) sum[j] = keysum[8 * k + j];
        if (!msm_key_fold(a, sum, c)) flags[k] = 1;
        for (int j = 0; j < 8; j++) sc[j * N + k] = a[j];
    }
    // digits: a host counting sort stands in for k_ed25519_keyeq_count / k_ed25519_batcheq_scan / k_ed25519_keyeq_scatter
    const size_t KB = (size_t)(wa + 1) * buckets;
    std::vector<std::vector<u32>> lists(KB);
    for (int w = 0; w <= wa; w++)
        for (size_t p = 0; p < N; p++) {
            const bool is_r = p >= K;
            const int dw = msm_window_digit(sh, w, is_r);
            if (dw < 0 || flags[p]) continue;
            const int d = msm_digit(&sc[p], N, dw, c, is_r ? wz : wa);
            if (d) lists[(size_t)w * buckets + msm_slot(sh, w, d < 0 ? -d : d, (u32)p)].push_back(((u32)p << 1) | (d < 0 ? 1u : 0u));
        }
    std::vector<u32> entries, begin(KB), end(KB);
    for (size_t k = 0; k < KB; k++) {
        begin[k] = (u32)entries.size();
        entries.insert(entries.end(), lists[k].begin(), lists[k].end());
        end[k] = (u32)entries.size();
    }
    entries.push_back(0);
    // buckets, windows (64 chunks per window, as the kernel's 64 lanes cut it), tail: the plain equation's
    std::vector<uint4> bk(KB * MSM_EXT_WORDS / 4), win((size_t)(wa + 1) * MSM_EXT_WORDS / 4);
    u32* bkw = reinterpret_cast<u32*>(bk.data());
    u32* winw = reinterpret_cast<u32*>(win.data());
    for (size_t k = 0; k < KB; k++) {
        ge_ext S;
        msm_bucket_sum(S, rows.data(), entries.data(), begin[k], end[k]);
        msm_store_ext(bkw + k * MSM_EXT_WORDS, S);
    }
    const u32 m = (u32)buckets / 64;
    for (int w = 0; w <= wa; w++) {
        ge_ext acc, t;
        msm_set_neutral(acc);
        for (u32 l = 0; l < 64; l++) {
            msm_chunk_sum(t, bkw + (size_t)w * buckets * MSM_EXT_WORDS, l * m, (l + 1) * m, msm_window_rlog2(sh, w));
            msm_ext_add(acc, t);
        }
        msm_store_ext(winw + (size_t)w * MSM_EXT_WORDS, acc);
    }
    ge_ext T, SB;
    msm_horner(T, winw, sh);
    u32 sw[8];
    msm_fold_s(sw, chunk);
    unsigned short cols[WB_COLS];
    wb_columns<true>(cols, 1, sw);
    ge_base_mult_wide<true>(SB, wide_tables(), cols, 1);
    msm_ext_add(T, SB);
    u32 enc[8];
    msm_encode(enc, T);
    wr32(point, 0, enc);
    return (msm_times8_is_neutral(T) && !reject) ? 1 : 0;
}

}  // extern "C"
