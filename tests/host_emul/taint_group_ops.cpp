// tests/host_emul/taint_group_ops.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over group_ops.cpp:
// ed25519_ScalarMult[_noclamp] at every window width and ed25519_ScalarMultBase[_noclamp].  Secret: the 32 scalar bytes.  Public:
// the points (an honest one, one of mixed order, one of small order, one that does not decode).  The wide comb counts as secret
// once built (taint_emul.cpp).  ed25519_PointAdd / PointSub handle no secret.
#include "group_ops.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    if (!args.base) return;
    constexpr size_t N = 5;
    // public points: [k]B for public k by the base call, B + T8 by the add call, a small-order encoding, an undecodable y
    std::vector<unsigned char> pub_k = taint::bytes(32 * N, 31), pts(32 * N), t8(32), tmp(32);
    std::vector<int> ok(N);
    emul_group_base(pts.data(), pub_k.data(), N, 0);
    memset(t8.data(), 0, 32);                                 // y = 0: a point of order 4
    emul_group_add(pts.data() + 32, ok.data(), pts.data() + 32, t8.data(), 1, 0);
    memcpy(pts.data() + 64, t8.data(), 32);
    memset(pts.data() + 96, 0, 32);
    pts[96] = 2;                                              // y = 2 is not on the curve
    for (int w = 2; w <= 4; w++)
        for (int clamp = 0; clamp < 2; clamp++)
            for (size_t n : { (size_t)1, N }) {
                std::vector<unsigned char> sc = taint::secret_bytes(32 * n, 32 + w), q(32 * n);
                taint::begin("scalarmult/w%d/%s/n%zu", w, clamp ? "clamped" : "noclamp", n);
                emul_group_scalarmult(q.data(), ok.data(), sc.data(), pts.data(), n, w, clamp);
            }
    wide_tables();
    taint::secret(g_wide);
    for (int clamp = 0; clamp < 2; clamp++)
        for (size_t n : { (size_t)1, N }) {
            std::vector<unsigned char> sc = taint::secret_bytes(32 * n, 41), q(32 * n);
            taint::begin("scalarmult_base/%s/n%zu", clamp ? "clamped" : "noclamp", n);
            emul_group_base(q.data(), sc.data(), n, clamp);
        }
}
