// curve25519_amd/csrc/scratch_carve.hpp -- how a *_dev call sizes its device scratch and cuts it into parts: ONE layout function per
// scratch shape, written against a Carve and run twice -- on a Carve without a base to learn the size of the lease, then on the leased
// slab to get the pointers (engine_common.cuh: lease_scratch).  A part cannot lie outside what was leased, because the same sequence of
// calls produced both.  A layout function does no pointer arithmetic of its own: in the sizing pass every part is null, and an offset from
// a part (its second word, say) is formed where the part is used, after the lease.  Host code with no HIP dependency:
// tests/c/scratch_carve_test.cpp runs it alone under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

// the projective result of a pass and the prefix products of its batched inversion: four parts of 10 n words, each rounded up to 4
// (16-byte aligned parts).  X25519 public_fast: a = numerator, z = denominator.  Edwards: a = X, b = Y, z = Z.
constexpr size_t SCR_FE = 10;
struct ProjScratch {
    uint32_t *a, *b, *z, *prefix;
};

namespace c25519_host {

class Carve {
public:
    Carve() = default;                                       // the sizing pass: offsets only, every part comes back null
    explicit Carve(void* slab) : base_(static_cast<unsigned char*>(slab)) {}
    uint32_t* take(size_t words)                             // the next `words` words
    {
        const size_t at = offset_;
        offset_ += words * sizeof(uint32_t);
        return base_ ? reinterpret_cast<uint32_t*>(base_ + at) : nullptr;
    }
    uint32_t* take4(size_t words) { return take((words + 3) / 4 * 4); }      // ... rounded up to 4 words: the next part stays 16-byte aligned
    void align(size_t bytes) { offset_ = (offset_ + bytes - 1) / bytes * bytes; }   // the next part begins on a multiple of `bytes` from the slab's start
    ProjScratch proj(size_t n)
    {
        ProjScratch p;
        p.a = take4(SCR_FE * n);
        p.b = take4(SCR_FE * n);
        p.z = take4(SCR_FE * n);
        p.prefix = take4(SCR_FE * n);
        return p;
    }
    size_t bytes() const { return offset_; }
    size_t words() const { return offset_ / sizeof(uint32_t); }

private:
    unsigned char* base_ = nullptr;
    size_t offset_ = 0;
};

}  // namespace c25519_host
