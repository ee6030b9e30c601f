// CPU check of gram4_claims.hpp (which bytes a region claim of gram4_kernels.hip stands for): for a grid of haystack lengths, large and
// small region sizes and split points, every claim index 0 .. nregions - 1 is walked through g4_claim_region and the regions must
//   * tile [0, vlen) exactly once, in ascending order: each begins where the one before ended, the last ends at vlen, none is empty;
//   * begin at a multiple of their own size, so that none straddles a multiple of 2 GiB (the kernel's epoch) — checked directly as well;
//   * be large below nlarge and small from there on, with the large part ending at a multiple of the large size;
// and the index one past the last must begin at or past vlen (a wave whose first index has no region reads nothing).
// Prints "OK plans=<n> regions=<n>" or the first failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../daachorse_amd/csrc/gram4_claims.hpp"

using namespace daac;

int main() {
    unsigned long long plans = 0, regions = 0;
    const uint64_t G2 = 1ull << 31;
    std::vector<uint64_t> larges = {2048, 4096, 65536, 262144, 1ull << 30};
    for (uint64_t large : larges) {
        std::vector<uint64_t> smalls = {2048, large / 2 >= 2048 ? large / 2 : 2048, large, large * 2};   // (above large: taken as large)
        if (large >= 65536) smalls.push_back(16384);
        // lengths around the region sizes, and — for regions large enough that the walk stays short — around 2 GiB and 4 GiB
        std::vector<uint64_t> vlens = {1, 15, 2047, 2048, 2049, large - 1, large, large + 1, 3 * large, 3 * large + 1, 7 * large + 2063,
                                       64 * large - 1, 64 * large + 15};
        if (large >= 65536) for (uint64_t v : {G2 - 1, G2, G2 + 1, G2 + 3 * large + 17, 2 * G2 + 5}) vlens.push_back(v);
        for (uint64_t vlen : vlens)
            for (uint64_t small : smalls) {
                if (vlen / (small < large ? small : large) > (1ull << 20)) continue;   // (keeps the walk short)
                const uint64_t all = (vlen + large - 1) / large;
                std::vector<uint64_t> splits = {0, large - 1, large, (all - 1) * large, all * large - 1, all * large, vlen, vlen + 1, (all + 3) * large, ~0ull};
                if (all > 2) splits.push_back((all / 2) * large + 5);
                if (vlen > G2) { splits.push_back(G2); splits.push_back(G2 - large); splits.push_back(G2 + large); }
                for (uint64_t split : splits) {
                    const G4Taper t = g4_taper_plan(vlen, large, small, split);
                    ++plans;
                    const uint64_t want_small = small < large ? small : large;
                    if (t.large != large || t.small != want_small || t.nlarge > t.nregions || t.nlarge > all || t.nregions == 0) {
                        std::printf("FAIL plan vlen=%llu large=%llu small=%llu split=%llu\n", (unsigned long long)vlen, (unsigned long long)large, (unsigned long long)small, (unsigned long long)split);
                        return 1;
                    }
                    if (split / large < all && t.nlarge != split / large) { std::printf("FAIL nlarge below the end\n"); return 1; }
                    if (split / large >= all && t.nlarge != all) { std::printf("FAIL nlarge past the end\n"); return 1; }
                    uint64_t at = 0;
                    for (uint64_t c = 0; c < t.nregions; ++c, ++regions) {
                        const G4Region r = g4_claim_region(c, t);
                        const uint64_t end = r.base + r.size < vlen ? r.base + r.size : vlen;
                        const bool ok = r.base == at && r.base < vlen && end > r.base && r.size == (c < t.nlarge ? t.large : t.small) &&
                                        (r.size & (r.size - 1)) == 0 && r.base % r.size == 0 && r.base / G2 == (end - 1) / G2;
                        if (!ok) {
                            std::printf("FAIL region vlen=%llu large=%llu small=%llu split=%llu claim=%llu base=%llu size=%llu expected base %llu\n", (unsigned long long)vlen,
                                        (unsigned long long)large, (unsigned long long)small, (unsigned long long)split, (unsigned long long)c, (unsigned long long)r.base,
                                        (unsigned long long)r.size, (unsigned long long)at);
                            return 1;
                        }
                        at = end;
                    }
                    if (at != vlen || g4_claim_region(t.nregions, t).base < vlen) {
                        std::printf("FAIL cover vlen=%llu large=%llu small=%llu split=%llu covered=%llu\n", (unsigned long long)vlen, (unsigned long long)large,
                                    (unsigned long long)small, (unsigned long long)split, (unsigned long long)at);
                        return 1;
                    }
                }
            }
    }
    std::printf("OK plans=%llu regions=%llu\n", plans, regions);
    return 0;
}
