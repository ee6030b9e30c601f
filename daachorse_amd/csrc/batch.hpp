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
    unsigned long long *rec;                  // MODE 3: one 8-byte record per reported match, the slot (output_pos - 1) in the low word
    unsigned long long *flags;                // [0] first decreasing offset, [1] first document on which leftmost + "" does not end
};

hipError_t launch_batch_plan(const unsigned long long *off, uint64_t n, uint64_t piece_bytes, unsigned long long *pieces, unsigned long long *flags,
                             hipStream_t stream);
hipError_t launch_batch_reduce(const unsigned long long *first, const unsigned long long *res, uint64_t n, unsigned long long *counts,
                               unsigned long long *checksums, hipStream_t stream);
hipError_t launch_batch_doc_offsets(const unsigned long long *first, const unsigned long long *piece_off, uint64_t n, const unsigned long long *total,
                                    unsigned long long *doc_off, hipStream_t stream);
// overlapping modes by piece on exactly one of the three engines; MODE 0 / 1 / 2 as for scan_kernel, MODE 3: slot records at rec + counts[piece]
hipError_t launch_batch_pieces(const TierDev *tier, const DArrayDev *da, const CharDev *chr, const BatchArgs &a, int mode, bool heads, uint32_t num_cu,
                               uint32_t threads, hipStream_t stream);
// chain modes, one lane per document of at most a.lane_max bytes, bytewise (da) or charwise (chr); kmode 3: slot records at rec + counts[doc]
hipError_t launch_batch_chain(const DArrayDev *da, const CharDev *chr, const BatchArgs &a, int kmode, bool leftmost, uint32_t num_cu, hipStream_t stream);

// ---- per-document pattern counts (daac_scan_histogram_batch, batch_hist_kernels.hip) ----
// Document i's records are rec[roff[i], roff[i+1]); the reduction leaves its rows {slot, count << 32}, in ascending slot order, at the
// front of that range and their number in rowcnt[i].  Three routes by the record count R: one wave a document (R <= wave_max), one
// workgroup a document (R <= sort_max) — both sort the slots in LDS and run-length encode them — and a dense counter row in HBM above.
constexpr uint32_t kBatchHistWaveCap = 4096;     // slots a wave sorts in its quarter of a 256-lane workgroup's 64 KB
constexpr uint32_t kBatchHistGroupCap = 32768;   // slots a workgroup sorts: the largest power of two that 160 KB of LDS hold
struct BatchHistArgs {
    unsigned long long *rec;
    const unsigned long long *roff;       // n + 1 record offsets
    uint64_t n;
    unsigned long long *rowcnt;           // n + 1: rows per document, rowcnt[n] = 0 (their exclusive scan is the call's doc_offsets)
    uint64_t wave_max, sort_max;          // clamped to the two caps
    unsigned long long *group_list;       // the documents of the workgroup route, in no particular order (n entries)
    unsigned long long *dense_list;       // ... and of the dense route
    unsigned long long *cls;              // [0] number of workgroup-route documents, [1] of dense ones, [2] first document longer than max_len
};
// classifies the documents by R, lists the workgroup-route and dense ones, checks the lengths against max_len and sets rowcnt[n] = 0
hipError_t launch_batch_hist_classify(const BatchHistArgs &h, const unsigned long long *off, uint64_t max_len, hipStream_t stream);
// the wave route over all documents (those above wave_max are skipped), or the workgroup route over group_list[0, items)
hipError_t launch_batch_hist_sort(const BatchHistArgs &h, bool wave, uint64_t items, uint32_t num_cu, hipStream_t stream);
// the dense route for dense_list[d0, d0 + nd): scratch holds nd rows of `slots` zeroed u32 counters
hipError_t launch_batch_hist_dense(const BatchHistArgs &h, uint32_t *scratch, uint64_t slots, uint64_t d0, uint32_t nd, hipStream_t stream);
// rows[doff[i] + r] = rec[roff[i] + r] for r < doff[i+1] - doff[i]: `total` = doff[n] rows
hipError_t launch_batch_hist_copy(const unsigned long long *rec, const unsigned long long *roff, const unsigned long long *doff, uint64_t n, uint64_t total,
                                  unsigned long long *rows, hipStream_t stream);

}  // namespace daac
