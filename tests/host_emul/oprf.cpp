// tests/host_emul/oprf.cpp -- TEST INFRASTRUCTURE.  The OPRF / VOPRF calls' lane functions (curve25519_amd/csrc/oprf25519.cuh) driven on
// the CPU the way engine_oprf.hip drives them: oprf_make_tail once per call as the host does it and one lane per row for the three
// per-row calls; for the two proof calls the three stages in turn over scratch arrays of the same shape -- the head lane, one lane
// per row (its request by oprf_owner), one lane per request (oprf_request, oprf_sum_rows, then the proof or the check) -- over the
// wide comb emul.cpp builds.  Built into its own library by tests/test_host_emul_oprf.py through tests/host_emul/build.py's open_lib.
// Not part of the product.
#include "emul.cpp"
#include "oprf25519.cuh"

namespace {

struct EmulPoints {
    std::vector<u32> x, y, z, t;
    explicit EmulPoints(size_t n) : x(10 * n + 1), y(10 * n + 1), z(10 * n + 1), t(10 * n + 1) {}
    OprfPoints view() { return OprfPoints{ x.data(), y.data(), z.data(), t.data() }; }
};

}  // namespace

extern "C" {

void emul_oprf_blind(unsigned char* blinded, int* ok, const unsigned char* input, size_t input_size, const unsigned char* blind, int mode, size_t n)
{
    H2cTail t;
    oprf_make_tail(t, input_size, (unsigned)mode);
    for (size_t i = 0; i < n; i++) {
        u32 bw[8], out[8];
        rd32(bw, blind, i);
        const u32 accept = oprf_blind_lane(out, input + i * input_size, t, bw);
        wr32(blinded, i, out);
        ok[i] = (int)(accept & 1u);
    }
}

void emul_oprf_finalize(unsigned char* output, int* ok, const unsigned char* input, size_t input_size, const unsigned char* blind,
                        const unsigned char* evaluated, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 bw[8], ew[8], out[16];
        rd32(bw, blind, i);
        rd32(ew, evaluated, i);
        const u32 accept = oprf_finalize_lane(out, input + i * input_size, input_size, bw, ew);
        memcpy(output + 64 * i, out, 64);
        ok[i] = (int)(accept & 1u);
    }
}

void emul_oprf_evaluate(unsigned char* evaluated, int* ok, const unsigned char* sks, const unsigned char* blinded, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        u32 kw[8], pw[8], out[8];
        rd32(kw, sks, 0);
        rd32(pw, blinded, i);
        const u32 accept = oprf_evaluate_lane(out, kw, pw);
        wr32(evaluated, i, out);
        ok[i] = (int)(accept & 1u);
    }
}

void emul_voprf_evaluate(unsigned char* evaluated, unsigned char* proof, int* ok, int* req_ok, const unsigned char* sks, const unsigned char* proof_rand,
                         const unsigned char* blinded, const unsigned long long* offsets, size_t m, size_t n)
{
    const u32* wide = wide_tables();
    EmulPoints pts(n);
    std::vector<u32> owner(n + 1), head(OPRF_HEAD_WORDS);
    unsigned short cols[WB_COLS];
    u32 kw[8];
    rd32(kw, sks, 0);
    {
        OprfHead h;
        oprf_server_head_lane(h, kw, wide, cols, 1);
        oprf_store_head(head.data(), h);
    }
    for (size_t i = 0; i < n; i++) {
        u32 idx, Dw[8];
        const u32 j = oprf_owner(idx, offsets, m, n, i);
        ge_ext term;
        const u32 accept = oprf_server_row_lane(Dw, term, kw, [&](u32 (&w)[8]) { rd32(w, blinded, i); },
                                                [&](u64 (&seed)[8]) { oprf_load_seed(seed, head.data()); }, idx, j == OPRF_NO_OWNER ? 0u : 0xffffffffu);
        wr32(evaluated, i, Dw);
        ok[i] = (int)(accept & 1u);
        oprf_store_point(pts.view(), n, i, term);
        owner[i] = (j & accept) | ~accept;
    }
    for (size_t j = 0; j < m; j++) {
        size_t lo;
        u32 count;
        u32 good = oprf_request(lo, count, offsets, j, n) ? 0xffffffffu : 0u;
        ge_ext M;
        good &= oprf_sum_rows(M, pts.view(), owner.data(), n, lo, count, (u32)j);
        OprfHead h;
        oprf_load_head(h, head.data());
        u32 rw[8], pf[16];
        rd32(rw, proof_rand, j);
        const u32 accept = oprf_prove_lane(pf, M, kw, rw, h, good, wide, cols, 1);
        memcpy(proof + 64 * j, pf, 64);
        req_ok[j] = (int)(accept & 1u);
    }
}

void emul_voprf_verify(int* req_ok, const unsigned char* pks, const unsigned char* blinded, const unsigned char* evaluated, const unsigned char* proof,
                       const unsigned long long* offsets, size_t m, size_t n)
{
    const u32* wide = wide_tables();
    EmulPoints pts_c(n), pts_d(n);
    std::vector<u32> owner(n + 1), owner_d(n + 1), head(OPRF_HEAD_WORDS);
    unsigned short cols[WB_COLS];
    {
        u32 pw[8];
        rd32(pw, pks, 0);
        OprfHead h;
        oprf_verifier_head_lane(h, pw);
        oprf_store_head(head.data(), h);
    }
    for (size_t lane = 0; lane < 2 * n; lane++) {
        const bool second = lane >= n;
        const size_t i = second ? lane - n : lane;
        u32 idx;
        const u32 j = oprf_owner(idx, offsets, m, n, i);
        ge_ext term;
        const u32 accept = oprf_verifier_point_lane(term, [&](u32 k, u32 (&w)[8]) { rd32(w, k ? evaluated : blinded, i); },
                                                    [&](u64 (&seed)[8]) { oprf_load_seed(seed, head.data()); }, idx, j == OPRF_NO_OWNER ? 0u : 0xffffffffu,
                                                    second ? 0xffffffffu : 0u);
        oprf_store_point(second ? pts_d.view() : pts_c.view(), n, i, term);
        (second ? owner_d : owner)[i] = (j & accept) | ~accept;
    }
    for (size_t j = 0; j < m; j++) {
        size_t lo;
        u32 count;
        u32 good = oprf_request(lo, count, offsets, j, n) ? 0xffffffffu : 0u;
        ge_ext M, Z;
        good &= oprf_sum_rows(M, pts_c.view(), owner.data(), n, lo, count, (u32)j);
        good &= oprf_sum_rows(Z, pts_d.view(), owner_d.data(), n, lo, count, (u32)j);
        OprfHead h;
        oprf_load_head(h, head.data());
        u32 pf[16];
        memcpy(pf, proof + 64 * j, 64);
        const u32 accept = oprf_check_lane(M, Z, pf, h, good, wide, cols, 1);
        req_ok[j] = (int)(accept & 1u);
    }
}

}  // extern "C"
