// tests/host_emul/taint_msm.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over msm.cpp: the constant-time path of
// ed25519_MultiScalarMult and ristretto255_MultiScalarMult (rows, chunked sum, finish) with m = 1 and 6 terms in 1 and 3 groups.
// Secret: the 32 bytes of every scalar.  Public: the points (any 32 bytes: a row that does not decode walks the same code and its
// group is masked, not skipped), m and n_groups.  The _vartime calls take public inputs only and are not run here.
#include "msm.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    if (!args.base) return;
    emul_msm_memoise = 0;
    for (int group = 0; group < 2; group++)
        for (size_t m : { (size_t)1, (size_t)6 })
            for (size_t n_groups : { (size_t)1, (size_t)3 }) {
                const size_t rows = m * n_groups;
                std::vector<unsigned char> sc = taint::secret_bytes(32 * rows, 61 + group), pts = taint::bytes(32 * rows, 62 + group), q(32 * n_groups);
                std::vector<int> ok(n_groups);
                for (size_t i = 0; i < rows; i++) pts[32 * i] &= 0xfe, pts[32 * i + 31] &= 0x3f;   // (ristretto255: even and below p)
                taint::begin("msm/%s/m%zu/g%zu", group ? "ristretto255" : "ed25519", m, n_groups);
                emul_msm_sum(q.data(), ok.data(), sc.data(), pts.data(), m, n_groups, group);
            }
}
