// normalize_batch on the device (daac_normalize_batch, daac_normalize, daac_spans_to_source): what api_normalize.hip and
// normalize_kernels.hip share.
//
// The definition (include/daachorse_amd.h has it in full).  A document is cut into the units of the splitter (split.hpp): a well-formed
// UTF-8 sequence (Unicode Table 3-7) that lies wholly inside the document is one unit with its code point, every other byte a unit of
// its own.  The output is, per document, the concatenation of the images of its units: a unit with a code point is looked up in the
// normalizer's table (copied, deleted, replaced by a string of the pool, padded with a space on either side, or decomposed as a Hangul
// syllable), a byte that is no well-formed sequence is copied.  `tokenizers` cannot be handed such bytes: it takes a str.  What a unit
// becomes depends on the unit alone, so the unit of parallelism is the byte: a count pass, an exclusive sum over the tiles, a write pass.
//
// Positions p count from offsets[0]: 0 <= p < total = offsets[n] - offsets[0].  The scratch of a call:
//   marks   one bit per position 0 .. total, as split.hpp has them (launch_split_marks sets them): a non-empty document starts here
//   counts  per tile: the bytes of the images of the units that start in the tile, then their exclusive sum
#pragma once

#include <cstdint>

#ifndef DAAC_NORMALIZE_HOST
#include <hip/hip_runtime.h>
#endif

namespace daac {

constexpr uint32_t kNormLanes = 256;       // lanes of a workgroup
constexpr uint32_t kNormPerLane = 4;       // consecutive positions of a lane
constexpr uint32_t kNormTile = kNormLanes * kNormPerLane;   // positions of a workgroup
constexpr int kNormBack = 3;               // bytes in front of a position its decision may read: the rest of a unit that holds it
constexpr int kNormAhead = 4;              // bytes from a position on its decision may read: a unit
constexpr uint32_t kNormStage1 = 0x1100;   // entries of the table's first stage: one per 256 code points up to U+10FFFF
constexpr uint32_t kNormBlock = 256;       // entries of a second-stage block
constexpr uint32_t kNormMaxLen = 255;      // the longest image of a REPLACE rule, in bytes
constexpr uint32_t kNormMaxPool = 1u << 21;   // bytes of a pool: an entry has 21 bits for the offset

// A table entry: the kind in bits 0 .. 2 (0: the unit is copied), a REPLACE image's length in bits 3 .. 10 and its offset in the pool in
// bits 11 .. 31.  The numbers of the kinds are daac_norm_kind's.
enum : uint32_t { kNormCopy = 0, kNormDelete = 1, kNormReplace = 2, kNormPad = 3, kNormHangul = 4 };
constexpr uint32_t kHangulFirst = 0xAC00u, kHangulLast = 0xD7A3u;

// The entry of a code point: ascii[cp] below U+0080 (the direct path), else stage2[stage1[cp >> 8] * 256 + (cp & 255)].  Block 0 is all
// copies.
struct NormTable {
    const uint32_t *ascii;    // 128 entries
    const uint16_t *stage1;   // kNormStage1 block numbers
    const uint32_t *stage2;   // blocks of kNormBlock entries
    const uint8_t *pool;
};

struct NormArgs {
    const uint8_t *text;                  // the byte at position 0 (offsets[0] of the caller's buffer), any alignment
    uint64_t total;                       // positions
    uint64_t base;                        // offsets[0]: what a position is counted from
    const unsigned long long *doc_off;    // n_docs + 1 offsets
    uint64_t n_docs;
    NormTable tab;
    const uint32_t *marks;                // tiles * kNormTile / 32 + 1 words
    unsigned long long *counts;           // tiles: the count pass's sums, then their exclusive sum
    const unsigned long long *out_len;    // 1: the sum of the counts
    uint64_t tiles;
    // the write pass
    uint8_t *out;                         // out_len bytes
    uint32_t *src;                        // out_len entries, or NULL
    unsigned long long *out_offsets;      // n_docs + 1
};

#ifndef DAAC_NORMALIZE_HOST
hipError_t launch_normalize_count(const NormArgs &a, hipStream_t stream);    // counts
hipError_t launch_normalize_write(const NormArgs &a, hipStream_t stream);    // out, src and out_offsets, behind the exclusive sum
// longest[0] = max(longest[0], the longest document's bytes): one lane per document
hipError_t launch_normalize_longest(const unsigned long long *doc_off, uint64_t n_docs, unsigned long long *longest, hipStream_t stream);
// {start, end} relative to the normalized document -> relative to the input document, in place: one lane per token
hipError_t launch_spans_to_source(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *out_offsets, const uint32_t *src,
                                  const uint8_t *hay, const unsigned long long *doc_off, uint64_t n_docs, uint64_t n_tokens, hipStream_t stream);
#endif

}  // namespace daac
