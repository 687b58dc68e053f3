// tests/c/scratch_carve_test.cpp -- csrc/scratch_carve.hpp alone, built with -fsanitize=address,undefined by
// tests/test_scratch_layout.py: the sizing pass and the carving pass of one sequence of take / take4 / align / proj calls end at the
// same offset, every part lies inside a slab of exactly the sized bytes, the parts are disjoint and aligned as asked, and the sizing
// pass hands out no pointer (it has no base to add to).  Every word of every part is written: a part that reached past the sized
// bytes would be a heap overflow under the address sanitizer.
#include "scratch_carve.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using c25519_host::Carve;

struct Part { uint32_t* p; size_t words; size_t align; };

// one layout with every kind of step, in the shape the engine's own have: a rounded part, an odd part, a projective part, a part
// behind a 256-byte boundary, a rounded tail
static void layout(Carve& c, size_t n, size_t m, std::vector<Part>& parts)
{
    parts.clear();
    parts.push_back({ c.take(32 * n), 32 * n, 16 });
    const ProjScratch s = c.proj(n);
    const size_t part = (SCR_FE * n + 3) / 4 * 4;
    parts.push_back({ s.a, part, 16 });
    parts.push_back({ s.b, part, 16 });
    parts.push_back({ s.z, part, 16 });
    parts.push_back({ s.prefix, part, 16 });
    parts.push_back({ c.take4(m), (m + 3) / 4 * 4, 16 });
    parts.push_back({ c.take(3), 3, 4 });
    parts.push_back({ c.take(m), m, 4 });
    c.align(256);
    parts.push_back({ c.take(8 * n), 8 * n, 256 });
    parts.push_back({ c.take4(n), (n + 3) / 4 * 4, 16 });
}

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s (n = %zu, m = %zu)\n", __FILE__, __LINE__, #cond, n, m); return 1; } \
    } while (0)

static int run(size_t n, size_t m)
{
    std::vector<Part> sized, cut;
    Carve size;
    layout(size, n, m, sized);
    for (const Part& p : sized) CHECK(p.p == nullptr);                       // no base, no pointer
    CHECK(size.bytes() == size.words() * sizeof(uint32_t));

    void* slab = aligned_alloc(256, (size.bytes() + 255) / 256 * 256);        // (aligned_alloc wants a multiple; only bytes() are touched)
    CHECK(slab != nullptr);
    Carve carve(slab);
    layout(carve, n, m, cut);
    CHECK(carve.bytes() == size.bytes());
    CHECK(cut.size() == sized.size());

    const unsigned char* lo = static_cast<const unsigned char*>(slab);
    const unsigned char* end = lo + size.bytes();
    const unsigned char* prev_end = lo;
    for (size_t k = 0; k < cut.size(); k++) {
        const Part& p = cut[k];
        CHECK(p.words == sized[k].words);
        const unsigned char* b = reinterpret_cast<const unsigned char*>(p.p);
        CHECK(b >= prev_end);                                                // in order and disjoint
        CHECK(b + p.words * sizeof(uint32_t) <= end);                        // inside what was sized
        CHECK(static_cast<size_t>(b - lo) % p.align == 0);
        for (size_t i = 0; i < p.words; i++) p.p[i] = (uint32_t)k;
        prev_end = b + p.words * sizeof(uint32_t);
    }
    CHECK(cut[0].p == static_cast<uint32_t*>(slab));                         // the first part is the slab's first byte
    for (size_t k = 0; k < cut.size(); k++)
        for (size_t i = 0; i < cut[k].words; i++) CHECK(cut[k].p[i] == (uint32_t)k);   // nobody wrote into a neighbour
    free(slab);
    return 0;
}

int main()
{
    const size_t sizes[] = { 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025 };
    for (size_t n : sizes)
        for (size_t m : sizes)
            if (run(n, m)) return 1;
    // sizing alone at the largest call the library takes: an offset, never an address
    Carve big;
    std::vector<Part> parts;
    layout(big, (size_t)1 << 26, ((size_t)1 << 26) + 1, parts);
    for (const Part& p : parts)
        if (p.p) return 1;
    if (big.bytes() % 4 != 0 || big.bytes() < ((size_t)1 << 26) * 32 * 4) return 1;
    puts("scratch_carve_test ok");
    return 0;
}
