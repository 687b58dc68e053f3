// tests/host_emul/msm.cpp -- TEST INFRASTRUCTURE.  The multiscalar calls' lane functions (curve25519_amd/csrc/msm_sum.cuh) driven on the
// CPU the way engine_msm.hip drives them per lane, on top of everything tests/host_emul/emul.cpp drives (this file includes it):
//   emul_msm_sum      the constant-time path: the rows stage, the chunked passes between two buffers, the finish;
//   emul_msm_bucket   the bucket path at width c, one group after the other: point rows, biased scalars, then a host counting sort in
//                     place of the count / scan / scatter kernels (as verify_batch.cpp does) with every point a "key", the bucket and
//                     window sums as the kernels' lanes cut them, the tail.
// group: 0 edwards25519, 1 ristretto255.  Built into its own library by tests/test_host_emul_msm.py through tests/host_emul/build.py's
// open_lib.  Not part of the product.
#include "emul.cpp"
#include "msm_sum.cuh"

#include <array>
#include <map>

// 0: every row runs the lane function (taint_msm.cpp: looking a SECRET scalar up in a map is the harness branching on it)
int emul_msm_memoise = 1;

namespace {

template <int G>
void sum_path(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups)
{
    const size_t rows = m * n_groups;
    std::vector<uint4> a(rows * MSM_EXT_WORDS / 4), b(((m + MSM_SUM_CHUNK - 1) / MSM_SUM_CHUNK) * n_groups * MSM_EXT_WORDS / 4 + 1);
    std::vector<u32> fa(rows), fb(b.size());
    u32 *src = reinterpret_cast<u32*>(a.data()), *dst = reinterpret_cast<u32*>(b.data()), *sflags = fa.data(), *dflags = fb.data();
    // k_msm_rows.  A walk costs ~3 ms under the C model and the cases draw points and scalars from small sets (tests/msm_model.py), so
    // the lane function runs once per distinct (scalar, point) pair of the call and its 40 words and flag are copied to the pair's
    // other rows: what the stages behind it read is the same.
    std::map<std::array<unsigned char, 64>, size_t> seen;
    for (size_t i = 0; i < rows; i++) {
        std::array<unsigned char, 64> key;
        if (emul_msm_memoise) {
            memcpy(key.data(), scalar + 32 * i, 32);
            memcpy(key.data() + 32, point + 32 * i, 32);
        }
        const auto hit = emul_msm_memoise ? seen.find(key) : seen.end();
        if (hit != seen.end()) {
            memcpy(src + i * MSM_EXT_WORDS, src + hit->second * MSM_EXT_WORDS, MSM_EXT_WORDS * sizeof(u32));
            sflags[i] = sflags[hit->second];
            continue;
        }
        if (emul_msm_memoise) seen[key] = i;
        u32 sw[8], pw[8];
        rd32(sw, scalar, i);
        rd32(pw, point, i);
        ge_ext S;
        sflags[i] = msm_sum_row_lane<G, MSM_WALK_WINDOW>(S, sw, pw);
        msm_store_ext(src + i * MSM_EXT_WORDS, S);
    }
    for (size_t m_in = m; m_in > 1;) {                       // k_msm_sum, pass by pass
        const size_t per = (m_in + MSM_SUM_CHUNK - 1) / MSM_SUM_CHUNK, total = per * n_groups;
        for (size_t t = 0; t < total; t++) {
            const size_t g = t / per, j = t - g * per, at = j * MSM_SUM_CHUNK;
            const u32 count = (u32)(m_in - at < (size_t)MSM_SUM_CHUNK ? m_in - at : (size_t)MSM_SUM_CHUNK);
            ge_ext S;
            dflags[t] = msm_sum_chunk_lane(S, src, sflags, g * m_in + at, count);
            msm_store_ext(dst + t * MSM_EXT_WORDS, S);
        }
        std::swap(src, dst);
        std::swap(sflags, dflags);
        m_in = per;
    }
    for (size_t g = 0; g < n_groups; g++) {                  // k_msm_finish (the Edwards inversion is the lane's own here)
        ge_ext S;
        msm_load_ext(S, src + g * MSM_EXT_WORDS);
        u32 out[8];
        msm_sum_encode<G>(out, S);
        for (int j = 0; j < 8; j++) out[j] &= sflags[g];
        wr32(q, g, out);
        ok[g] = (int)(sflags[g] & 1u);
    }
}

template <int G>
void bucket_path(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups, int c)
{
    const MsmShape sh = msm_shape(c);
    const int wa = sh.wa, buckets = sh.buckets;
    const size_t K = (size_t)wa * buckets;
    for (size_t g = 0; g < n_groups; g++) {
        std::vector<uint4> rowbuf(m * MSM_ROW_WORDS / 4);
        u32* rows = reinterpret_cast<u32*>(rowbuf.data());
        std::vector<u32> sc(8 * m), flags(m, 0);
        bool reject = false;
        for (size_t j = 0; j < m; j++) {                     // k_msm_points, k_msm_scalars
            u32 w[8], row[24], k[8];
            rd32(w, point, g * m + j);
            if (!msm_sum_point_row<G>(row, w)) { flags[j] = 1; reject = true; }
            memset(rows + j * MSM_ROW_WORDS, 0, MSM_ROW_WORDS * sizeof(u32));
            memcpy(rows + j * MSM_ROW_WORDS, row, sizeof row);
            rd32(w, scalar, g * m + j);
            msm_sum_biased_scalar(k, w, c);
            for (int i = 0; i < 8; i++) sc[i * m + j] = k[i];
        }
        std::vector<std::vector<u32>> lists(K);              // count / scan / scatter: every point a key
        for (int w = 0; w < wa; w++)
            for (size_t p = 0; p < m; p++) {
                if (flags[p]) continue;
                const int d = msm_digit(&sc[p], m, msm_window_digit(sh, w, false), c, wa);
                if (d) lists[(size_t)w * buckets + msm_slot(sh, w, d < 0 ? -d : d, (u32)p)].push_back(((u32)p << 1) | (d < 0 ? 1u : 0u));
            }
        std::vector<u32> entries, begin(K), end(K);
        for (size_t k = 0; k < K; k++) {
            begin[k] = (u32)entries.size();
            entries.insert(entries.end(), lists[k].begin(), lists[k].end());
            end[k] = (u32)entries.size();
        }
        entries.push_back(0);
        std::vector<uint4> bk(K * MSM_EXT_WORDS / 4), win((size_t)wa * MSM_EXT_WORDS / 4);
        u32* bkw = reinterpret_cast<u32*>(bk.data());
        u32* winw = reinterpret_cast<u32*>(win.data());
        for (size_t k = 0; k < K; k++) {                     // buckets
            ge_ext S;
            msm_bucket_sum(S, rows, entries.data(), begin[k], end[k]);
            msm_store_ext(bkw + k * MSM_EXT_WORDS, S);
        }
        const u32 per = (u32)buckets / 64;
        for (int w = 0; w < wa; w++) {                       // windows: 64 chunks, as the kernel's lanes cut them
            ge_ext acc, t;
            msm_set_neutral(acc);
            for (u32 l = 0; l < 64; l++) {
                msm_chunk_sum(t, bkw + (size_t)w * buckets * MSM_EXT_WORDS, l * per, (l + 1) * per, msm_window_rlog2(sh, w));
                msm_ext_add(acc, t);
            }
            msm_store_ext(winw + (size_t)w * MSM_EXT_WORDS, acc);
        }
        ge_ext T;                                            // k_msm_tail
        msm_sum_horner(T, winw, sh);
        u32 out[8];
        msm_sum_encode<G>(out, T);
        for (int j = 0; j < 8; j++) out[j] &= reject ? 0u : 0xffffffffu;
        wr32(q, g, out);
        ok[g] = reject ? 0 : 1;
    }
}

}  // namespace

extern "C" {

void emul_msm_sum(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups, int group)
{
    if (group) sum_path<MSM_GROUP_R255>(q, ok, scalar, point, m, n_groups);
    else sum_path<MSM_GROUP_EDWARDS>(q, ok, scalar, point, m, n_groups);
}

void emul_msm_bucket(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups, int group, int c)
{
    if (group) bucket_path<MSM_GROUP_R255>(q, ok, scalar, point, m, n_groups, c);
    else bucket_path<MSM_GROUP_EDWARDS>(q, ok, scalar, point, m, n_groups, c);
}

int emul_msm_chunk(void) { return MSM_SUM_CHUNK; }

}  // extern "C"
