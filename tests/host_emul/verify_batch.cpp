// tests/host_emul/verify_batch.cpp -- TEST INFRASTRUCTURE.  The lane-level code of the ZIP-215 batch equation
// (curve25519_amd/csrc/msm25519.cuh: scalars, point rows, signed digits, bucket sums, window sums, the tail) compiled for the host
// against the C model of the gfx950 primitives, on top of everything tests/host_emul/emul.cpp drives (this file includes it).  What the
// kernels of engine_batch_eq.hip do across lanes -- the counting sort with atomics, the reductions -- is done here by plain host loops:
//   emul_batcheq_digits   the signed digits of one scalar at width c (as an a_i or as a z_i); emul_batcheq_top_range: its top window's R;
//   emul_batcheq          the whole chain for one call: enc(T) as the hook returns it, and the result.
// Built into its own library by tests/test_host_emul_verify_batch.py through tests/host_emul/build.py's build_lib.
// Not part of the product.
#include "emul.cpp"
#include "msm25519.cuh"

extern "C" {

// digits[0 .. return value): the signed digits of the 32-byte little-endian scalar; as_z: the windows of a 128-bit scalar
int emul_batcheq_digits(int* digits, const unsigned char* scalar, int c, int as_z)
{
    u32 k[8];
    rd32(k, scalar, 0);
    const int nwin = as_z ? msm_windows_z(c) : msm_windows_a(c);
    msm_bias(k, c, nwin);
    for (int w = 0; w < nwin; w++) digits[w] = msm_digit(k, 1, w, c, nwin);
    return nwin;
}

// R of the scalar's top window: the sub-bucket range its digit must stay within (msm_slot)
int emul_batcheq_top_range(int c, int as_z) { const MsmShape sh = msm_shape(c); return 1 << (as_z ? sh.rz : sh.ra); }

// point: 32 bytes, enc(T) over the elements that pass rules 1-3; returns the result of the call
int emul_batcheq(unsigned char* point, const unsigned char* sig, const unsigned char* pk, const unsigned char* msg, size_t len, size_t n,
                 const unsigned char* seed, int c)
{
    const size_t N = 2 * n;
    const MsmShape sh = msm_shape(c);
    const int wa = sh.wa, wz = sh.wz, buckets = sh.buckets;
    u32 seedw[8];
    rd32(seedw, seed, 0);
    std::vector<u32> rows(N * MSM_ROW_WORDS, 0), sc(8 * N), flags(n, 0);
    // points (k_ed25519_batcheq_points)
    for (size_t j = 0; j < N; j++) {
        u32 w[8], row[24];
        if (j >= n) rd32(w, sig, 2 * (j - n)); else rd32(w, pk, j);
        if (!msm_point_row(row, w)) flags[j >= n ? j - n : j] = 1;
        memcpy(&rows[j * MSM_ROW_WORDS], row, sizeof row);
    }
    // scalars (k_ed25519_batcheq_scalars): the s_i leave as sums of 16-bit chunks
    u64 chunk[16] = {};
    for (size_t i = 0; i < n; i++) {
        u32 pkw[8], Rw[8], Sw[8], a[8], z[8], s[8];
        rd32(pkw, pk, i);
        rd32(Rw, sig, 2 * i);
        rd32(Sw, sig, 2 * i + 1);
        if (!msm_scalars(a, z, s, pkw, Rw, Sw, msg + len * i, len, seedw, i, c)) flags[i] = 1;
        for (int j = 0; j < 8; j++) { sc[j * N + i] = a[j]; sc[j * N + n + i] = z[j]; }
        if (flags[i]) continue;
        for (int j = 0; j < 16; j++) chunk[j] += (s[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    }
    bool reject = false;
    for (size_t i = 0; i < n; i++) reject = reject || flags[i];
    // digits: a host counting sort stands in for k_ed25519_batcheq_count / _scan / _scatter
    const size_t K = (size_t)(wa + 1) * buckets;
    std::vector<std::vector<u32>> lists(K);
    for (int w = 0; w <= wa; w++)
        for (size_t p = 0; p < N; p++) {
            const bool is_r = p >= n;
            const int dw = msm_window_digit(sh, w, is_r);
            if (dw < 0 || flags[is_r ? p - n : p]) continue;
            const int d = msm_digit(&sc[p], N, dw, c, is_r ? wz : wa);
            if (d) lists[(size_t)w * buckets + msm_slot(sh, w, d < 0 ? -d : d, (u32)p)].push_back(((u32)p << 1) | (d < 0 ? 1u : 0u));
        }
    std::vector<u32> entries, begin(K), end(K);
    for (size_t k = 0; k < K; k++) {
        begin[k] = (u32)entries.size();
        entries.insert(entries.end(), lists[k].begin(), lists[k].end());
        end[k] = (u32)entries.size();
    }
    entries.push_back(0);
    // buckets, windows (64 chunks per window, as the kernel's 64 lanes cut it), tail
    std::vector<uint4> bk(K * MSM_EXT_WORDS / 4), win((size_t)(wa + 1) * MSM_EXT_WORDS / 4);
    u32* bkw = reinterpret_cast<u32*>(bk.data());
    u32* winw = reinterpret_cast<u32*>(win.data());
    for (size_t k = 0; k < K; k++) {
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
