// tests/host_emul/taint_oprf.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over oprf.cpp, at every input length the
// run names (one whose bytes straddle a word behind the two length bytes of Finalize's string, one that ends on a word) with one
// row and six, and for the VOPRF server with one request and with three over six rows:
//   blind      ristretto255_OPRF_Blind: input and blind secret
//   finalize   ristretto255_OPRF_Finalize: input and blind secret (evaluated is what the server sent: public)
//   evaluate   ristretto255_OPRF_BlindEvaluate: skS secret
//   voprf      ristretto255_VOPRF_BlindEvaluate: skS and every proof_rand secret
// Public: the lengths, the mode, blinded, offsets, the counts and indices.  The wide comb counts as secret once built
// (taint_group_ops.cpp).  ristretto255_VOPRF_VerifyProof handles no secret.
#include "oprf.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    constexpr size_t N = 6;
    wide_tables();
    taint::secret(g_wide);
    // (the public rows are any even 32 bytes below p: a row that does not decode walks the same code and is masked, not skipped)
    for (size_t len : args.lens)
        for (size_t n : { (size_t)1, N }) {
            std::vector<unsigned char> input = taint::secret_bytes(len * n + 1, 200 + len), blind = taint::secret_bytes(32 * n, 201 + len);
            std::vector<unsigned char> blinded(32 * n), out(64 * n);
            std::vector<int> ok(n);
            taint::begin("blind/len%zu/n%zu", len, n);
            emul_oprf_blind(blinded.data(), ok.data(), input.data(), len, blind.data(), (int)(len & 1), n);
            taint::open(blinded);                               // published
            taint::begin("finalize/len%zu/n%zu", len, n);
            emul_oprf_finalize(out.data(), ok.data(), input.data(), len, blind.data(), blinded.data(), n);
        }
    if (!args.base) return;
    for (size_t n : { (size_t)1, N }) {
        std::vector<unsigned char> sks = taint::secret_bytes(32, 210), blinded = taint::bytes(32 * n, 211), evaluated(32 * n);
        std::vector<int> ok(n);
        for (size_t i = 0; i < n; i++) blinded[32 * i] &= 0xfe, blinded[32 * i + 31] &= 0x3f;      // even and below p: the decoder's first two rules
        taint::begin("evaluate/n%zu", n);
        emul_oprf_evaluate(evaluated.data(), ok.data(), sks.data(), blinded.data(), n);
        const size_t m = n == 1 ? 1 : 3;
        const unsigned long long offsets[4] = { 0, n == 1 ? 1ull : 2ull, 3, N };
        std::vector<unsigned char> rnd = taint::secret_bytes(32 * m, 212), proof(64 * m);
        std::vector<int> req_ok(m);
        taint::begin("voprf/n%zu", n);
        emul_voprf_evaluate(evaluated.data(), proof.data(), ok.data(), req_ok.data(), sks.data(), rnd.data(), blinded.data(), offsets, m, n);
    }
}
