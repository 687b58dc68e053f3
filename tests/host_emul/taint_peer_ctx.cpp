// tests/host_emul/taint_peer_ctx.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over peer_ctx.cpp: X25519 against
// many peer contexts in one call.  Secret: sk.  Public: the peer keys, ctx_index, and every context's key and eligibility word
// (which sends an element to the comb or to the ladder list).  The contexts' rows are public as well, but count as secret once
// built, so that what a secret column selects from them stays tainted.
#include "peer_ctx.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    if (!args.base) return;
    constexpr size_t N_CTX = 4;
    std::vector<unsigned char> pk = taint::bytes(32 * N_CTX, 81), ctxs(PEER_CTX_BYTES * N_CTX);
    emul_peer_init(ctxs.data(), pk.data(), N_CTX);
    size_t eligible = 0;
    for (size_t c = 0; c < N_CTX; c++) {
        u32 flag;
        memcpy(&flag, ctxs.data() + PEER_CTX_BYTES * c + 4 * PEER_CTX_ELIGIBLE, 4);
        eligible += flag == 1u;
        taint::secret(ctxs.data() + PEER_CTX_BYTES * c + 4 * PEER_CTX_ROWS, PEER_CTX_BYTES - 4 * PEER_CTX_ROWS);
    }
    if (eligible == 0 || eligible == N_CTX) abort();         // both the comb and the ladder list must run
    for (size_t n : { (size_t)1, (size_t)5 }) {
        std::vector<unsigned> index(n);
        for (size_t i = 0; i < n; i++) index[i] = (unsigned)((i + n) % N_CTX);
        std::vector<unsigned char> sk = taint::secret_bytes(32 * n, 82), out(32 * n);
        taint::begin("peer_indexed/lane/n%zu", n);
        emul_peer_indexed(out.data(), ctxs.data(), N_CTX, index.data(), sk.data(), n);
    }
    // one element against each context alone, so that a context of either kind is walked whatever the seeds give
    for (size_t c = 0; c < N_CTX; c++) {
        const unsigned index = (unsigned)c;
        std::vector<unsigned char> sk = taint::secret_bytes(32, 83 + c), out(32);
        taint::begin("peer_indexed/lane/ctx%zu/n1", c);
        emul_peer_indexed(out.data(), ctxs.data(), N_CTX, &index, sk.data(), 1);
    }
}
