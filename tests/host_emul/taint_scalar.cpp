// tests/host_emul/taint_scalar.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over scalar.cpp: ed25519_ScalarInvert at
// every group size (one element, and K + 1: a whole group and a ragged one), ed25519_ScalarMul, _ScalarMulAdd, _ScalarAdd, _ScalarSub,
// _ScalarNegate, _ScalarComplement and _ScalarReduce.  Secret: every scalar input byte.  Public: the element count and index.
#include "scalar.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    if (!args.base) return;
    for (int k : { 1, 2, 4, 8, 16 })
        for (size_t n : { (size_t)1, (size_t)k + 1 }) {
            std::vector<unsigned char> s = taint::secret_bytes(32 * n, 50 + k), recip(32 * n);
            std::vector<int> ok(n);
            taint::begin("invert/k%d/n%zu", k, n);
            emul_scalar_invert(recip.data(), ok.data(), s.data(), n, k);
        }
    constexpr size_t N = 6;
    const struct { const char* name; int op; int inputs; size_t width; } calls[] = {
        { "mul", SC_OP_MUL, 2, 32 }, { "muladd", SC_OP_MULADD, 3, 32 }, { "add", SC_OP_ADD, 2, 32 }, { "sub", SC_OP_SUB, 2, 32 },
        { "negate", SC_OP_NEGATE, 1, 32 }, { "complement", SC_OP_COMPLEMENT, 1, 32 }, { "reduce", SC_OP_REDUCE, 1, 64 },
    };
    for (const auto& call : calls)
        for (size_t n : { (size_t)1, N }) {
            std::vector<unsigned char> a = taint::secret_bytes(call.width * n, 70 + call.op), b = taint::secret_bytes(32 * n, 80 + call.op),
                                       c = taint::secret_bytes(32 * n, 90 + call.op), r(32 * n);
            taint::begin("%s/n%zu", call.name, n);
            emul_scalar_op(call.op, r.data(), a.data(), call.inputs > 1 ? b.data() : nullptr, call.inputs > 2 ? c.data() : nullptr, n);
        }
}
