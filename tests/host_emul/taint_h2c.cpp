// tests/host_emul/taint_h2c.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over h2c.cpp: ed25519_HashToCurve,
// ed25519_EncodeToCurve, ristretto255_HashToGroup and ed25519_HashToScalar at every message length the run names (one whose last
// word straddles message and tail, one word-aligned) with one element and six, ed25519_MapToCurve, and c25519_ExpandMessageXmd.
// Secret: the message bytes, the 32 bytes of u.  Public: the lengths, the DST, the element count and index.
#include "h2c.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    constexpr size_t N = 6;
    const std::vector<unsigned char> dst = taint::bytes(45, 61);
    const char* names[] = { "hash_to_curve", "encode_to_curve", "hash_to_group", "hash_to_scalar" };
    for (size_t len : args.lens)
        for (size_t n : { (size_t)1, N }) {
            for (int call = 0; call < 4; call++) {
                std::vector<unsigned char> msg = taint::secret_bytes(len * n + 1, 100 + call), p(32 * n);
                taint::begin("%s/len%zu/n%zu", names[call], len, n);
                emul_h2c_call(call, p.data(), msg.data(), len, dst.data(), dst.size(), n);
            }
            std::vector<unsigned char> msg = taint::secret_bytes(len * n + 1, 104), out(129 * n);
            taint::begin("expand/len%zu/n%zu", len, n);
            emul_h2c_expand(out.data(), msg.data(), len, dst.data(), dst.size(), 129, n);
        }
    if (!args.base) return;
    for (size_t n : { (size_t)1, N }) {
        std::vector<unsigned char> u = taint::secret_bytes(32 * n, 67), p(32 * n);
        if (n == N) {                                         // the exceptional input among them: u = 0, still marked
            taint::open(u);
            memset(u.data() + 32, 0, 32);
            taint::secret(u);
        }
        taint::begin("map/n%zu", n);
        emul_h2c_map(p.data(), u.data(), n);
    }
}
