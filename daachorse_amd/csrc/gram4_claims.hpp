// gram4_claims.hpp — which bytes a claim of the `.count()` kernel stands for (host and device).
//
// The haystack [0, vlen) is cut into regions that the waves of a launch claim one after the other from a counter (gram4_kernels.hip).
// Two sizes, both powers of two: the first `nlarge` regions are `large` bytes, what lies behind them is cut into regions of `small <=
// large` bytes, the last of them as long as the haystack leaves it.  The large part ends at a multiple of `large`, so every region
// starts at a multiple of its own size and none straddles a multiple of 2 GiB (the kernel's epoch: regions are at most 1 GiB).
// The small regions at the end are what evens out the waves' finish times: a wave that ends early takes a few more of them instead of
// waiting for the one that got the last large region.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define G4C_HD __host__ __device__ __forceinline__
#else
#define G4C_HD inline
#endif

namespace daac {

struct G4Taper {
    uint64_t large = 0, small = 0;   // region sizes in bytes, powers of two, small <= large
    uint64_t nlarge = 0;             // claims [0, nlarge) are large regions
    uint64_t nregions = 0;           // all claims
};
struct G4Region {
    uint64_t base;   // first byte
    uint64_t size;   // the region's full size (large or small); the bytes it holds: min(size, vlen - base)
};

// `split`: the byte the small regions begin at, rounded down here to a multiple of `large`; at or past the end: large regions only.
inline G4Taper g4_taper_plan(uint64_t vlen, uint64_t large, uint64_t small, uint64_t split) {
    G4Taper t;
    t.large = large;
    t.small = small < large ? small : large;
    const uint64_t all_large = (vlen + large - 1) / large;
    t.nlarge = split / large < all_large ? split / large : all_large;
    const uint64_t behind = t.nlarge * large < vlen ? vlen - t.nlarge * large : 0;
    t.nregions = t.nlarge + (behind + t.small - 1) / t.small;
    return t;
}

// claim index -> region (wave-uniform arithmetic on the device: the sizes as their logarithms, so an index becomes bytes by shifts)
G4C_HD uint32_t g4_log2(uint64_t pow2) {
    uint32_t l = 0;
    while ((1ull << l) < pow2) ++l;
    return l;
}
G4C_HD G4Region g4_claim_region(uint64_t claim, uint32_t large_log2, uint32_t small_log2, uint64_t nlarge) {
    if (claim < nlarge) return G4Region{claim << large_log2, 1ull << large_log2};
    return G4Region{(nlarge << large_log2) + ((claim - nlarge) << small_log2), 1ull << small_log2};
}
G4C_HD G4Region g4_claim_region(uint64_t claim, const G4Taper &t) { return g4_claim_region(claim, g4_log2(t.large), g4_log2(t.small), t.nlarge); }

}  // namespace daac
