// tests/host_emul/taint_vrf.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over vrf.cpp: ed25519_VRF_Prove at
// every alpha length the run names (one whose bytes straddle a word behind the 32 key bytes, one word-aligned) with one element and
// six.  Secret: the 32 seed bytes of every private key -- and with them SHA-512(seed), x, k and what s is computed from.  Public: the
// key's other half (Prove reads it as given: any 32 bytes serve), alpha, the lengths, the element count and index.  The wide comb
// counts as secret once built (taint_group_ops.cpp).  ed25519_VRF_Verify and ed25519_VRF_ProofToHash handle no secret.
#include "vrf.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    constexpr size_t N = 6;
    wide_tables();
    taint::secret(g_wide);
    for (size_t len : args.lens)
        for (size_t n : { (size_t)1, N }) {
            std::vector<unsigned char> priv = taint::bytes(64 * n, 93 + len), alpha = taint::bytes(len * n + 1, 94 + len), proof(80 * n);
            for (size_t i = 0; i < n; i++) taint::secret(priv.data() + 64 * i, 32);
            taint::begin("prove/len%zu/n%zu", len, n);
            emul_vrf_prove(proof.data(), priv.data(), alpha.data(), len, n);
        }
}
