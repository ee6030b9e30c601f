// The batch scanners (batch_kernels.hip) as the host driver (api_batch.hip) sees them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_tables.hpp"

namespace daac {

struct BatchArgs {
    const uint8_t *hay;                       // byte 0 of the buffer
    const unsigned long long *off;            // n + 1 document offsets
    uint64_t n;
    const unsigned long long *first_piece;    // overlapping modes: n + 1 entries, first_piece[n] = npieces
    uint64_t npieces;
    uint64_t piece_bytes;
    uint32_t halo;
    uint64_t lane_max;                        // chain modes: longer documents are left to the host driver
    unsigned long long *res;                  // MODE 0: 3 x u64 {count, S1, S2} per piece (overlapping) / per document (chain)
    unsigned long long *counts;               // MODE 1 out, MODE 2 in (exclusive offsets): per piece / per document
    uint4 *out;                               // MODE 2: daac_match16 {end lo, end hi, length, value}
    unsigned long long *flags;                // [0] first decreasing offset, [1] first document on which leftmost + "" does not end
};

hipError_t launch_batch_plan(const unsigned long long *off, uint64_t n, uint64_t piece_bytes, unsigned long long *pieces, unsigned long long *flags,
                             hipStream_t stream);
hipError_t launch_batch_reduce(const unsigned long long *first, const unsigned long long *res, uint64_t n, unsigned long long *counts,
                               unsigned long long *checksums, hipStream_t stream);
hipError_t launch_batch_doc_offsets(const unsigned long long *first, const unsigned long long *piece_off, uint64_t n, const unsigned long long *total,
                                    unsigned long long *doc_off, hipStream_t stream);
// overlapping modes by piece on exactly one of the three engines; MODE 0 / 1 / 2 as for scan_kernel
hipError_t launch_batch_pieces(const TierDev *tier, const DArrayDev *da, const CharDev *chr, const BatchArgs &a, int mode, bool heads, uint32_t num_cu,
                               uint32_t threads, hipStream_t stream);
// chain modes, one lane per document of at most a.lane_max bytes, bytewise (da) or charwise (chr)
hipError_t launch_batch_chain(const DArrayDev *da, const CharDev *chr, const BatchArgs &a, int kmode, bool leftmost, uint32_t num_cu, hipStream_t stream);

}  // namespace daac
