// granule.h -- internal: the self-validating 8-byte output granule, for host and device code alike.
// A double leaves the device as TWO granules {tag << 32 | 32 bits of the double}, low half first; a reader re-reads the pair
// until both carry the tag of the evaluation it waits for ("the data IS the flag": no separate flag word, no store drain).
// The tag of sequence number seq is seq % (2^32 - 1) + 1: never 0, which is what an empty (zeroed) buffer holds.
#pragma once

#if defined(__HIP__)
#define CFMM_GRANULE_FN __host__ __device__ __forceinline__
#else
#define CFMM_GRANULE_FN inline
#endif

namespace cfmm {

CFMM_GRANULE_FN unsigned long long granule_tag(unsigned long long seq) { return seq % 0xffffffffull + 1ull; }

// half 0 / 1 of the 64 bits `u` of a double under `tag`
CFMM_GRANULE_FN unsigned long long granule_of_bits(unsigned long long tag, unsigned long long u, int half)
{
    return (tag & 0xffffffffull) << 32 | (half ? u >> 32 : u & 0xffffffffull);
}
CFMM_GRANULE_FN unsigned long long granule(unsigned long long tag, double x, int half)
{
    unsigned long long u;
    __builtin_memcpy(&u, &x, sizeof u);
    return granule_of_bits(tag, u, half);
}

// the pair {a, b} = {low, high}: false unless BOTH carry `tag`; else x is the double they hold
CFMM_GRANULE_FN bool granule_join(unsigned long long a, unsigned long long b, unsigned long long tag, double& x)
{
    if ((a >> 32) != tag || (b >> 32) != tag) return false;
    const unsigned long long u = (a & 0xffffffffull) | (b << 32);
    __builtin_memcpy(&x, &u, sizeof x);
    return true;
}

} // namespace cfmm
