// tests/host_emul/taint_harness.h -- TEST INFRASTRUCTURE.  The shared part of the secret-taint programs (taint_*.cpp: one per
// emulation unit, each with its own main through taint_main below; built with MemorySanitizer by tests/host_emul/build.py's
// build_taint, run as subprocesses by tests/test_secret_taint.py, never loaded into python).  A case marks the SECRET inputs of one
// operation uninitialised (__msan_poison) and calls the unit's emul_* entry point: MemorySanitizer then reports every branch
// whose condition, and every load or store whose address, derives from a secret, in the device source the unit compiles.  A value
// loaded THROUGH a secret address gets the shadow of the memory it came from, so the tables the secret indexes are poisoned too
// (after they are built): a row of a clean table would be clean and the rest of the walk unchecked.
// The program prints "@@CASE <name>" on stderr in front of each case; the reports between two markers are that case's.
#pragma once
#include <sanitizer/msan_interface.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace taint {

inline void secret(void* p, size_t bytes) { __msan_poison(p, bytes); }
inline void open(void* p, size_t bytes) { __msan_unpoison(p, bytes); }
template <typename T> void secret(std::vector<T>& v) { secret(v.data(), v.size() * sizeof(T)); }
template <typename T> void open(std::vector<T>& v) { open(v.data(), v.size() * sizeof(T)); }

// (no std::string here or in the units' cases: libstdc++'s own code is not instrumented and leaves stale shadow behind)
__attribute__((format(printf, 1, 2))) inline void begin(const char* fmt, ...)
{
    open(&c25519::emul_mad_overflows, sizeof c25519::emul_mad_overflows);      // (the counter adds up secret-derived carries)
    char name[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof name, fmt, ap);
    va_end(ap);
    fprintf(stderr, "@@CASE %s\n", name);
}

// n deterministic bytes (xorshift64*), public until a case says otherwise
inline std::vector<unsigned char> bytes(size_t n, uint64_t seed)
{
    std::vector<unsigned char> v(n);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
    for (size_t i = 0; i < n; i++) {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        v[i] = (unsigned char)((s * 0x2545F4914F6CDD1Dull) >> 56);
    }
    return v;
}

inline std::vector<unsigned char> secret_bytes(size_t n, uint64_t seed)
{
    std::vector<unsigned char> v = bytes(n, seed);
    secret(v);
    return v;
}

struct Args {
    bool base = false;                              // run the cases that take no message
    std::vector<size_t> lens;                       // message lengths of the signing cases
    const char *invert_zero = nullptr, *invert_plain = nullptr;        // files of limbs for the shared inversion (tests/invert_cases.py: make_inputs)
    size_t invert_n = 0;
    int invert_k = 0;
};

// ---- the self-check of the method: four lane functions with a known answer (tests/test_secret_taint.py asserts each) ------------
namespace self {

using c25519::u32;
using c25519::u64;

__attribute__((noinline)) u32 extra_work(u32 x)
{
    u64 acc = x;
    for (int i = 0; i < 8; i++) acc = c25519::mad64(acc, (u32)acc | 1u, 0x9E3779B9u) >> 7;
    return (u32)acc;
}

// 1: a branch on a secret bit -- must be reported as a branch
__attribute__((noinline)) u32 selfcheck_branch(const u32* k, u32 x)
{
    if (k[0] & 1u) x = extra_work(x);
    return x;
}

// 2: an array indexed by a secret byte -- must be reported as an address, in a function no list allows
__attribute__((noinline)) u32 selfcheck_index(const u32* k, const u32* table256)
{
    return table256[k[0] & 0xffu];
}

// 3: a branch on a field of a row fetched by secret index -- a branch report only if the TABLE is poisoned (the row's shadow is
// the table's, not the index's)
__attribute__((noinline)) u32 selfcheck_row_branch(const u32* k, const u32* table16x4, u32 x)
{
    const u32* row = table16x4 + 4 * (k[0] & 15u);
    if (row[1] & 1u) x = extra_work(x);
    return x;
}

// 4: a select by mask -- must be silent
__attribute__((noinline)) u32 selfcheck_select(const u32* k, u32 a, u32 b)
{
    const u32 m = 0u - (k[0] & 1u);
    return (a & m) | (b & ~m);
}

inline void run(bool poison_table)
{
    std::vector<unsigned char> kb = bytes(32, 1);
    kb[0] |= 1;
    u32 k[8], table[256];
    memcpy(k, kb.data(), 32);
    for (int i = 0; i < 256; i++) table[i] = 2 * i + 1;
    volatile u32 sink;
    secret(k, sizeof k);
    begin("selfcheck_branch");
    sink = selfcheck_branch(k, 5);
    begin("selfcheck_index");
    sink = selfcheck_index(k, table);
    if (poison_table) secret(table, sizeof table);
    begin("selfcheck_row_branch");
    sink = selfcheck_row_branch(k, table, 5);
    begin("selfcheck_select");
    sink = selfcheck_select(k, 3, 4);
    (void)sink;
}

}  // namespace self

}  // namespace taint

// every unit defines this: its cases, each behind taint::begin(name)
static void taint_cases(const taint::Args& args);

// <program> selfcheck [clean-table] | <program> cases <base,len,len,...> [<zero.bin> <plain.bin> <n> <k>]
int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "selfcheck")) {
        taint::self::run(!(argc >= 3 && !strcmp(argv[2], "clean-table")));
        fprintf(stderr, "@@END\n");
        return 0;
    }
    if (argc < 3 || strcmp(argv[1], "cases")) {
        fprintf(stderr, "usage: %s selfcheck | cases <lengths> [<zero limbs> <plain limbs> <n> <k>]\n", argv[0]);
        return 2;
    }
    taint::Args args;
    for (const char* p = argv[2]; *p;) {                       // "base" and message lengths, comma-separated: one run can take a share
        if (!strncmp(p, "base", 4)) {
            args.base = true;
            p += 4;
        } else {
            char* end;
            args.lens.push_back(strtoul(p, &end, 10));
            p = end;
        }
        if (*p) p++;
    }
    if (argc >= 7) {
        args.invert_zero = argv[3];
        args.invert_plain = argv[4];
        args.invert_n = strtoul(argv[5], nullptr, 10);
        args.invert_k = atoi(argv[6]);
    }
    taint_cases(args);
    taint::open(&c25519::emul_mad_overflows, sizeof c25519::emul_mad_overflows);
    fprintf(stderr, "@@END overflows=%llu\n", c25519::emul_mad_overflows);
    return 0;
}
