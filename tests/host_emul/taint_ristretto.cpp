// tests/host_emul/taint_ristretto.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over ristretto.cpp:
// ristretto255_ScalarMult at every window width (decode and encode included), ristretto255_ScalarMultBase and ristretto255_FromHash.
// Secret: the 32 scalar bytes, the 64 hash bytes.  Public: the points (valid ones, the identity, one of every class that does not
// decode).  The wide comb counts as secret once built (taint_emul.cpp).  IsValidPoint, PointAdd and PointSub handle no secret.
#include "ristretto.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    if (!args.base) return;
    constexpr size_t N = 6;
    // public points: FromHash of public strings, the identity, a non-canonical s, an odd s, an s without a square root
    std::vector<unsigned char> pub_h = taint::bytes(64 * N, 29), pts(32 * N);
    std::vector<int> ok(N), valid(N);
    emul_rist_from_hash(pts.data(), pub_h.data(), N);
    memset(pts.data() + 32, 0, 32);                           // the identity
    memset(pts.data() + 64, 0xff, 32);                        // s >= p
    memset(pts.data() + 96, 0, 32);
    pts[96] = 1;                                              // s odd
    for (unsigned char c = 2; c < 64; c += 2) {               // the first small even s that does not decode
        memset(pts.data() + 128, 0, 32);
        pts[128] = c;
        emul_rist_is_valid(valid.data(), pts.data() + 128, 1);
        if (!valid[0]) break;
    }
    for (int w = 2; w <= 4; w++)
        for (size_t n : { (size_t)1, N }) {
            std::vector<unsigned char> sc = taint::secret_bytes(32 * n, 32 + w), q(32 * n);
            taint::begin("scalarmult/w%d/n%zu", w, n);
            emul_rist_scalarmult(q.data(), ok.data(), sc.data(), pts.data(), n, w);
        }
    for (size_t n : { (size_t)1, N }) {
        std::vector<unsigned char> h = taint::secret_bytes(64 * n, 43), p(32 * n);
        taint::begin("from_hash/n%zu", n);
        emul_rist_from_hash(p.data(), h.data(), n);
    }
    wide_tables();
    taint::secret(g_wide);
    for (size_t n : { (size_t)1, N }) {
        std::vector<unsigned char> sc = taint::secret_bytes(32 * n, 41), q(32 * n);
        taint::begin("scalarmult_base/n%zu", n);
        emul_rist_base(q.data(), sc.data(), n);
    }
}
