// tests/host_emul/taint_key_convert.cpp -- TEST INFRASTRUCTURE.  Secret-taint cases (taint_harness.h) over key_convert.cpp:
// ed25519_PrivateKey_to_X25519.  Secret: priv[0..31].  The public-key calls of the unit (classification, conversion of public
// keys) handle no secret.
#include "key_convert.cpp"
#include "taint_harness.h"

static void taint_cases(const taint::Args& args)
{
    if (!args.base) return;
    for (size_t n : { (size_t)1, (size_t)5 }) {
        std::vector<unsigned char> priv = taint::bytes(64 * n, 71), xsk(32 * n);
        for (size_t i = 0; i < n; i++) taint::secret(priv.data() + 64 * i, 32);
        taint::begin("private_to_x25519/lane/n%zu", n);
        emul_key_private_to_x25519(xsk.data(), priv.data(), n);
    }
}
