// Per-pattern match counts of an overlapping scan (daac_scan_histogram): what api_hist.hip and hist_kernels.hip share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_tables.hpp"

namespace daac {

// LDS of a workgroup of the histogram scan: the engine's own tables (TIERED: its staged tiers, DARRAY: ROOT's row, charwise: none), then
// `lds_bins` 32-bit counters for the first slots.
constexpr uint32_t kHistLdsLimit = 160u * 1024u;
inline uint32_t hist_engine_lds(const TierDev *tier, const DArrayDev *da) {
    return tier ? ((tier->lds_bytes + 15u) & ~15u) : da ? 256u * 16u : 0u;
}

struct HistArgs {
    uint32_t *heads;     // one counter per output record ("slot"), zero on entry: hits whose state's list starts at the record
    uint32_t n;          // number of slots
    uint32_t lds_bins;   // slots [0, lds_bins) are counted in LDS per workgroup and flushed at its end
    uint32_t off_bins;   // where they lie in LDS (behind the engine's tables)
};

// exactly one of tier / da / chr is set; a.begin .. a.len is the launch's range (shorter than 2^32 bytes: a counter takes one hit per position)
hipError_t launch_hist_scan(const TierDev *tier, const DArrayDev *da, const CharDev *chr, const ScanArgs &a, const HistArgs &h, uint32_t blocks,
                            uint32_t threads, hipStream_t stream);
// counts[i] += heads[i]; heads[i] = 0
hipError_t launch_hist_fold(uint32_t *heads, unsigned long long *counts, uint64_t n, hipStream_t stream);
// counts[ancestor] += snap[i] for every record i with snap[i] != 0 and every ancestor on i's parent chain (outputs: n x {value, length, parent})
hipError_t launch_hist_propagate(const uint32_t *outputs, const unsigned long long *snap, unsigned long long *counts, uint64_t n, hipStream_t stream);

}  // namespace daac
