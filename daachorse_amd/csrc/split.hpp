// split_batch on the device (daac_split_batch, daac_split, daac_offsets_compose): what api_split.hip and split_kernels.hip share.
//
// The definition (include/daachorse_amd.h has it in full).  A document is cut into units: a well-formed UTF-8 sequence (Unicode
// Table 3-7) that lies wholly inside the document is one unit of its code point's class, every other byte a unit of class O.  The
// classes are L, N, S and O; below U+0080 they are fixed, from U+0080 on they come from the splitter's ranges.  The words of a
// document are the successive matches of \s+|\S+ (DAAC_SPLIT_WHITESPACE) or of GPT-2's pattern (DAAC_SPLIT_GPT2) over the units, or
// BERT's pre-tokenizer words with the whitespace runs between them (DAAC_SPLIT_BERT): contiguous, covering the document.  Whether a word starts at a byte is decided from the bytes of its document at most kSplitBack
// before it and kSplitAhead - 1 after it (split_kernels.hip has the local form), so the unit of parallelism is the byte.
// DAAC_SPLIT_CL100K and DAAC_SPLIT_LLAMA3 read four more bits of a position that depend on runs of any length (a digit's index in its
// run mod 3, newlines behind punctuation, a newline farther on in a whitespace run, a whitespace run that reaches the document's end):
// segmented scans over the batch, two forwards and two backwards, in three passes that never wait for one another (split_kernels.hip).
// DAAC_SPLIT_O200K has the same three passes with states of its own: forwards one automaton of 13 states, backwards two bits.
//
// Positions p count from offsets[0]: 0 <= p < total = offsets[n] - offsets[0].  The scratch of a call:
//   marks   one bit per position 0 .. total: a non-empty document starts here (bit `total`: the text ends here); set with atomicOr
//   masks   one bit per position, kSplitTile / 64 words of 64 per tile: a word starts here
//   counts  per tile: the set bits of its masks; their exclusive sum ranks the word starts
// and for the two rules with scans, 12 bytes a tile:
//   tile_sum  per tile: what the tile does to each of the four scan states, as a packed function (kSum* below)
//   carry_f   per tile: the forward states in front of the tile's first position (kFwd*)
//   carry_b   per tile: the backward states behind the tile's last position (kBwd*)
#pragma once

#include <cstdint>

#ifndef DAAC_SPLIT_HOST
#include <hip/hip_runtime.h>
#endif

namespace daac {

constexpr uint32_t kSplitLanes = 256;    // lanes of a workgroup
constexpr uint32_t kSplitTile = 1024;    // positions of a workgroup: kSplitTile / kSplitLanes per lane, one ballot each
constexpr int kSplitBack = 12;           // bytes in front of a position its decision may read: three units of four bytes
constexpr int kSplitAhead = 8;           // bytes from a position on its decision may read: the position and seven more
constexpr uint32_t kSplitStage1 = 0x1100;   // entries of the class table's first stage: one per 256 code points up to U+10FFFF
constexpr uint32_t kSplitBlockBytes = 64;   // a second-stage block: 256 code points, two bits each

enum : uint32_t { kSplitO = 0, kSplitL = 1, kSplitN = 2, kSplitS = 3 };
// DAAC_SPLIT_O200K: three classes more, and L is then a caseless letter.  Its table has four bits per code point in blocks of
// kSplitBlockBytes4: (stage2[stage1[cp >> 8] * 128 + ((cp & 255) >> 1)] >> 4 * (cp & 1)) & 15.
enum : uint32_t { kSplitUp = 4, kSplitLow = 5, kSplitMark = 6 };
constexpr uint32_t kSplitBlockBytes4 = 128;
constexpr uint32_t kSplitCarryLanes = 1024;   // lanes of the one workgroup that resolves the carries across tiles

// A scan state is a function of the positions in front of (forwards) or behind (backwards) a position; a position either keeps the
// state it is handed or sets it.  What a word of 64 positions, a tile or a span of tiles does to the four states, packed:
enum : uint32_t {
    kSumKeepD = 1u << 0, kSumAddD = 3u << 1,   // y' = ((keep ? y : 0) + add) % 3: the units of a digit run so far, mod 3
    kSumKeepT = 1u << 3, kSumValT = 1u << 4,   // x' = keep ? x : val: an O unit, then only newlines
    kSumKeepF = 1u << 5, kSumValF = 1u << 6,   // f' likewise, backwards: whitespace as far as a newline
    kSumKeepE = 1u << 7, kSumValE = 1u << 8,   // e' likewise, backwards: whitespace as far as the document's end
    kSumFwd = kSumKeepD | kSumAddD | kSumKeepT | kSumValT,
    kSumBwd = kSumKeepF | kSumValF | kSumKeepE | kSumValE,
    kSumIdentity = kSumKeepD | kSumKeepT | kSumKeepF | kSumKeepE,
};
// the states themselves: forwards y | x << 2, backwards f | e << 1

// The class of a code point from U+0080 on: (stage2[stage1[cp >> 8] * 64 + ((cp & 255) >> 2)] >> 2 * (cp & 3)) & 3.  Block 0 is all O.
struct SplitTable {
    const uint16_t *stage1;   // kSplitStage1 block numbers
    const uint8_t *stage2;    // blocks of kSplitBlockBytes
};

struct SplitArgs {
    const uint8_t *text;                  // the byte at position 0 (offsets[0] of the caller's buffer), any alignment
    uint64_t total;                       // positions
    uint64_t base;                        // offsets[0]: what a position is counted from
    const unsigned long long *doc_off;    // n_docs + 1 offsets
    uint64_t n_docs;
    int rule;
    SplitTable tab;
    uint32_t *marks;                      // tiles * kSplitTile / 32 + 1 words
    unsigned long long *masks;            // tiles * kSplitTile / 64 words
    unsigned long long *counts;           // tiles: the flag pass's counts, then their exclusive sum
    const unsigned long long *n_words;    // 1: the sum of the counts
    uint64_t tiles;
    // DAAC_SPLIT_CL100K and DAAC_SPLIT_LLAMA3 only: tiles entries each
    uint32_t *tile_sum;
    uint32_t *carry_f;
    uint32_t *carry_b;
    // the write passes
    unsigned long long *word_offsets;     // n_words + 1
    unsigned long long *doc_words;        // n_docs + 1
};

// DAAC_SPLIT_O200K: the arguments of its own passes.  Scratch per tile, 20 bytes: tile_map (what the tile does to the forward state, a
// packed map of 16 states), a.tile_sum (what it does to the two backward bits), a.carry_f (the forward state in front of the tile) and
// a.carry_b (the backward bits behind it).  split_kernels.hip has the states.
struct SplitO200kArgs {
    SplitArgs a;
    unsigned long long *tile_map;   // tiles entries
};

#ifndef DAAC_SPLIT_HOST
hipError_t launch_split_flags_o200k(const SplitO200kArgs &a, hipStream_t stream);   // tile_map and tile_sum, the carries, then masks and counts
hipError_t launch_split_marks(const SplitArgs &a, hipStream_t stream);     // marks (zeroed by the caller)
hipError_t launch_split_flags(const SplitArgs &a, hipStream_t stream);     // masks and counts
// DAAC_SPLIT_CL100K / DAAC_SPLIT_LLAMA3: tile_sum, then carry_f and carry_b, then masks and counts
hipError_t launch_split_flags_scanned(const SplitArgs &a, hipStream_t stream);
hipError_t launch_split_scatter(const SplitArgs &a, hipStream_t stream);   // word_offsets and doc_words, the closing entries included
// out[i] = inner[outer[i]] for i < n
hipError_t launch_offsets_compose(const unsigned long long *inner, const unsigned long long *outer, uint64_t n, unsigned long long *out, hipStream_t stream);
// spans of a word batch's tokens, relative to the word, made relative to the word's document: one lane per word
hipError_t launch_spans_rebase(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *word_offsets,
                               const unsigned long long *doc_words, const unsigned long long *doc_off, uint64_t n_words, uint64_t n_docs, hipStream_t stream);
// flags[w] = 1 iff the word [word_offsets[w], word_offsets[w+1]) of `text` (the byte that offset 0 names) is not empty and its first unit is
// of class S; a word that is not inside [lo, hi) gets 0 and none of its bytes is read: one lane per word.  o200k: tab is DAAC_SPLIT_O200K's
hipError_t launch_split_words_space(const SplitTable &tab, const uint8_t *text, const unsigned long long *word_offsets, uint64_t n_words, uint64_t lo, uint64_t hi,
                                    uint8_t *flags, hipStream_t stream, bool o200k = false);
#endif

}  // namespace daac
