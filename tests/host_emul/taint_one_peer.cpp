// tests/host_emul/taint_one_peer.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over one_peer.cpp: X25519 against
// one remembered peer key.  Secret: sk.  Public: the peer key, and with it the peer's eligibility, which chooses between the comb
// and the ladder for the whole call.  The peer's comb is public too, but counts as secret once built, so that the rows a secret
// column selects stay tainted; it is built from a public copy of the secrets (the model generates only the rows a call selects).
#include "one_peer.cpp"
#include "taint_harness.h"

namespace {

// the first seeded peer key that is (not) eligible for the comb
std::vector<unsigned char> peer_key(bool eligible)
{
    for (uint64_t seed = 1;; seed++) {
        std::vector<unsigned char> pk = taint::bytes(32, 100 + seed);
        u32 u[8], q[3][8];
        rd32(u, pk.data(), 0);
        if ((x25519_peer_point(q, u) != 0) == eligible) return pk;
    }
}

void comb_case(size_t n)
{
    const std::vector<unsigned char> pk = peer_key(true);
    std::vector<unsigned char> sk = taint::bytes(32 * n, 61), out(32 * n);
    u32 u[8], q[3][8];
    rd32(u, pk.data(), 0);
    if (!x25519_peer_point(q, u)) abort();
    std::vector<u32> k(8 * n), wide_peer;
    for (size_t i = 0; i < n; i++) {
        u32 w[8];
        rd32(w, sk.data(), i);
        clamp_words(w);
        memcpy(&k[8 * i], w, 32);
    }
    one_peer_needed_rows(wide_peer, q, k, n);
    taint::secret(wide_peer);
    taint::secret(k);
    taint::begin("one_peer/comb/n%zu", n);
    std::vector<unsigned short> cols(WB_COLS * n);
    for (size_t i = 0; i < n; i++) {                         // emul_one_peer's walk and finish
        u32 kw[8], w[8];
        memcpy(kw, &k[8 * i], 32);
        fe num, den, zi;
        x25519_one_peer_lane(num, den, kw, wide_peer.data(), &cols[WB_COLS * i], 1);
        fe_invert(zi, den);
        fe_mul(num, num, zi);
        fe_to_words(w, num);
        wr32(out.data(), i, w);
    }
}

}  // namespace

static void taint_cases(const taint::Args& args)
{
    if (!args.base) return;
    for (size_t n : { (size_t)1, (size_t)5 }) {
        comb_case(n);
        const std::vector<unsigned char> pk = peer_key(false);
        std::vector<unsigned char> sk = taint::secret_bytes(32 * n, 62), out(32 * n);
        taint::begin("one_peer/ladder/n%zu", n);
        if (emul_one_peer(out.data(), pk.data(), sk.data(), n) != 0) abort();
    }
}
