// replace_all on the device (daac_replace_all, daac_replace_all_batch): what api_replace.hip and replace_kernels.hip share.
//
// The input is the ordered, non-overlapping list of 16-byte tuples {end u64, length u32, value u32} of find_iter / leftmost_find_iter
// (a batch: the CSR list, ends relative to the document).  With the exclusive sums R_i of the replacement lengths and L_i of the match
// lengths, the replacement of match i begins at output position O_i = start_i - L_i + R_i = end_i - L_{i+1} + R_i, non-decreasing in i.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace daac {

constexpr uint32_t kSpliceLanes = 256;                 // lanes of a splice workgroup, 16 output bytes each
constexpr uint32_t kSpliceTile = kSpliceLanes * 16;    // output bytes a workgroup writes per turn
constexpr uint32_t kSpliceStage = 1536;                // segments that begin inside a tile and whose positions are staged in LDS (6 KB);
                                                       // a tile with more (ties, or text denser than three matches per eight bytes) searches HBM

struct ReplaceArgs {
    const uint8_t *hay;               // byte 0 of the text (a batch: of document 0)
    uint64_t len;                     // bytes of text
    uint4 *seg;                       // k tuples; the sizing pass rewrites each as {end lo, end hi (in the text), rlen, position of the replacement in the blob}
    uint64_t k;
    unsigned long long *rpre;         // k + 1: rlen_i, then R_i (entry k: the total), then O_i
    unsigned long long *lpre;         // k + 1: length_i, then L_i
    const uint8_t *repl;              // the replacements' bytes
    uint64_t repl_bytes;
    const unsigned long long *roff;   // n_repl + 1 offsets into them
    uint64_t n_repl;                  // 1: every match takes replacement 0; otherwise a match takes replacement `value`
    unsigned long long *bad;          // the first match whose value has no replacement (~0: none)
    // batches (n_docs != 0): the tuple list's CSR offsets and the documents' offsets
    const unsigned long long *doc_first;   // n_docs + 1
    const unsigned long long *doc_off;     // n_docs + 1
    uint64_t n_docs;
    // the splice
    uint8_t *out;                     // 16-byte aligned
    uint64_t out_len;
    long long *tile_lo;               // tiles + 1: the last segment that begins at or before the tile's first byte (-1: none), entry `tiles`: k - 1
    uint64_t tiles;
};

// one lane per match: replacement index (and the bad-value flag), rlen_i and length_i for the sums, the tuple rewritten in place
hipError_t launch_replace_size(const ReplaceArgs &a, hipStream_t stream);
// a batch's out_offsets[d] = (doc_off[d] - doc_off[0]) - L[doc_first[d]] + R[doc_first[d]], after the sums and before replace_finish
hipError_t launch_replace_doc_offsets(const ReplaceArgs &a, unsigned long long *out_offsets, hipStream_t stream);
// rpre[i] = O_i, after the sums
hipError_t launch_replace_finish(const ReplaceArgs &a, hipStream_t stream);
// tile_lo (one lane per tile: a binary search in O), then the splice itself
hipError_t launch_replace_splice(const ReplaceArgs &a, uint32_t num_cu, hipStream_t stream);

}  // namespace daac
