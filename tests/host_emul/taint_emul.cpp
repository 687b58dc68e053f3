// tests/host_emul/taint_emul.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over emul.cpp: X25519, public keys,
// Ed25519 key pairs and signatures, plain and blinded, Blinding_Init and the shared inversion, on every form emul.cpp drives (one
// lane, quads, one wave, two waves; the 8 x 32 comb and the wide comb).  Secret: sk / seed, priv[0..31], the 192-byte blinding
// context and its seed, the values to invert.  Public: peer keys, messages, lengths, priv[32..63].
#include "emul.cpp"
#include "taint_harness.h"

namespace {

using taint::begin;
using taint::bytes;
using taint::secret_bytes;
typedef std::vector<unsigned char> buf;

const size_t LANE_N[] = { 1, 5 };
constexpr size_t QUAD_N = quad::ELEMS_PER_WAVE, WAVE_N = 1;

// the tables every fixed-base walk fetches from count as secret from here on: what a secret column selects stays tainted
void poison_tables()
{
    tables();
    wide_tables();
    taint::secret(g_tbl);
    taint::secret(g_wide);
}

// priv[n][64] with a real public half, by emul_ed25519_keypair on public seeds while the tables are still public (clean_priv: made
// once per size, in front of poison_tables); a case takes a copy with priv[0..31] of every row secret
std::vector<buf> g_clean_priv;

void prepare_priv()
{
    emul_set_base_comb(0);
    for (size_t n : { LANE_N[0], LANE_N[1], QUAD_N }) {
        buf sk = bytes(32 * n, 50 + n), pub(32 * n), priv(64 * n);
        emul_ed25519_keypair(pub.data(), priv.data(), nullptr, sk.data(), n);
        g_clean_priv.push_back(priv);
    }
}

buf make_priv(size_t n)
{
    for (const buf& p : g_clean_priv)
        if (p.size() == 64 * n) {
            buf priv = p;
            for (size_t i = 0; i < n; i++) taint::secret(priv.data() + 64 * i, 32);
            return priv;
        }
    abort();
}

void x25519_cases()
{
    for (int fixed = 0; fixed < 2; fixed++) {                     // against a peer key; the public key by the ladder (pk == NULL)
        const char* tag = fixed ? "x25519_public_ladder" : "x25519";
        for (size_t n : LANE_N) {
            buf pk = bytes(32 * n, 11), sk = secret_bytes(32 * n, 12), out(32 * n);
            begin("%s/lane/n%zu", tag, n);
            emul_x25519(out.data(), fixed ? nullptr : pk.data(), sk.data(), n);
        }
        {
            buf pk = bytes(32 * QUAD_N, 13), sk = secret_bytes(32 * QUAD_N, 14), out(32 * QUAD_N);
            begin("%s/quad/n%zu", tag, QUAD_N);
            emul_quad_x25519(out.data(), fixed ? nullptr : pk.data(), sk.data(), QUAD_N);
        }
        {
            buf pk = bytes(32 * WAVE_N, 15), sk = secret_bytes(32 * WAVE_N, 16), out(32 * WAVE_N);
            begin("%s/wave/n%zu", tag, WAVE_N);
            emul_coop_x25519(out.data(), fixed ? nullptr : pk.data(), sk.data(), WAVE_N);
        }
        if (!fixed) {                                              // (the two-wave form always reads a peer key)
            buf pk = bytes(32 * WAVE_N, 17), sk = secret_bytes(32 * WAVE_N, 18), out(32 * WAVE_N);
            begin("%s/two_waves/n%zu", tag, WAVE_N);
            emul_coop_x25519_two_waves(out.data(), fixed ? nullptr : pk.data(), sk.data(), WAVE_N);
        }
    }
}

void public_fast_cases()
{
    for (int wide = 0; wide < 2; wide++) {
        emul_set_base_comb(wide);
        for (size_t n : LANE_N) {
            buf sk = secret_bytes(32 * n, 21), pk(32 * n);
            begin("x25519_public/lane/%s/n%zu", wide ? "wide" : "comb", n);
            emul_x25519_public_fast(pk.data(), sk.data(), n);
        }
        buf sk = secret_bytes(32 * WAVE_N, 22), pk(32 * WAVE_N);
        begin("x25519_public/wave/%s/n%zu", wide ? "wide" : "comb", WAVE_N);
        emul_coop_public_fast(pk.data(), sk.data(), WAVE_N, wide);
    }
    buf sk = secret_bytes(32 * QUAD_N, 23), pk(32 * QUAD_N);
    begin("x25519_public/quad/wide/n%zu", QUAD_N);
    emul_quad_public_fast(pk.data(), sk.data(), QUAD_N);
}

// Blinding_Init by the lane and by the wave; returns the wave's context
buf blinding_cases()
{
    buf ctx(4 * BLIND_WORDS), ctx_wave(4 * BLIND_WORDS);
    for (size_t len : { (size_t)32, (size_t)64 }) {
        buf seed = secret_bytes(len, 31 + len);
        begin("blinding_init/lane/n1/len%zu", len);
        emul_blinding_init(ctx.data(), seed.data(), len);
        begin("blinding_init/wave/n1/len%zu", len);
        emul_coop_blinding_init(ctx_wave.data(), seed.data(), len);
    }
    return ctx_wave;
}

void keypair_cases(const buf& blinding)
{
    for (int wide = 0; wide < 2; wide++)
        for (int blind = 0; blind < 2; blind++) {
            emul_set_base_comb(wide);
            const char* form = wide ? (blind ? "wide/blinded" : "wide") : (blind ? "comb/blinded" : "comb");
            for (size_t n : LANE_N) {
                buf sk = secret_bytes(32 * n, 41), pub(32 * n), priv(64 * n);
                begin("keypair/lane/%s/n%zu", form, n);
                emul_ed25519_keypair(pub.data(), priv.data(), blind ? blinding.data() : nullptr, sk.data(), n);
            }
            if (blind && !wide) continue;                          // the wave blinds over the wide comb only
            buf sk = secret_bytes(32 * WAVE_N, 42), pub(32 * WAVE_N), priv(64 * WAVE_N);
            begin("keypair/wave/%s/n%zu", form, WAVE_N);
            emul_coop_keypair(pub.data(), priv.data(), blind ? blinding.data() : nullptr, sk.data(), WAVE_N, wide);
        }
    buf sk = secret_bytes(32 * QUAD_N, 43), pub(32 * QUAD_N), priv(64 * QUAD_N);
    begin("keypair/quad/wide/n%zu", QUAD_N);
    emul_quad_keypair(pub.data(), priv.data(), sk.data(), QUAD_N);
}

void sign_cases(const buf& blinding, size_t len)
{
    for (int wide = 0; wide < 2; wide++)
        for (int blind = 0; blind < 2; blind++) {
            emul_set_base_comb(wide);
            const char* form = wide ? (blind ? "wide/blinded" : "wide") : (blind ? "comb/blinded" : "comb");
            for (size_t n : LANE_N) {
                buf priv = make_priv(n), msg = bytes(len * n + 1, 52), sig(64 * n);
                begin("sign/lane/%s/n%zu/len%zu", form, n, len);
                emul_ed25519_sign(sig.data(), priv.data(), blind ? blinding.data() : nullptr, msg.data(), len, n);
            }
            if (blind && !wide) continue;
            buf priv = make_priv(WAVE_N), msg = bytes(len * WAVE_N + 1, 54), sig(64 * WAVE_N);
            begin("sign/wave/%s/n%zu/len%zu", form, WAVE_N, len);
            emul_coop_sign(sig.data(), priv.data(), blind ? blinding.data() : nullptr, msg.data(), len, WAVE_N, wide);
        }
    buf priv = make_priv(QUAD_N), msg = bytes(len * QUAD_N + 1, 56), sig(64 * QUAD_N);
    begin("sign/quad/wide/n%zu/len%zu", QUAD_N, len);
    emul_quad_sign(sig.data(), priv.data(), msg.data(), len, QUAD_N);
}

void invert_case(const char* name, const char* path, size_t n, int k)
{
    std::vector<unsigned> in(10 * n), out(8 * n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    taint::secret(in);
    begin("%s/n%zu/k%d", name, n, k);
    emul_batch_invert(out.data(), in.data(), n, k);
}

}  // namespace

static void taint_cases(const taint::Args& args)
{
    if (args.base) {
        x25519_cases();
        if (args.invert_zero) {
            invert_case("invert/zero_slot", args.invert_zero, args.invert_n, args.invert_k);
            invert_case("invert/no_zero", args.invert_plain, args.invert_n, args.invert_k);
        }
    }
    prepare_priv();
    buf blinding(4 * BLIND_WORDS);
    if (!args.base) {                                              // a run of signing cases alone: the context they use, made while the tables are public
        buf seed = bytes(64, 31 + 64);
        emul_coop_blinding_init(blinding.data(), seed.data(), 64);
    }
    poison_tables();
    if (args.base) {
        public_fast_cases();
        blinding = blinding_cases();
    }
    taint::secret(blinding);
    if (args.base) keypair_cases(blinding);
    for (size_t len : args.lens) sign_cases(blinding, len);
}
