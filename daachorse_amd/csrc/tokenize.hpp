// tokenize on the device (daac_tokenize, daac_tokenize_batch): what api_tokenize.hip and tokenize_kernels.hip share.
//
// The input is the text and the ordered, non-overlapping list of 16-byte tuples {end u64, length u32, value u32} of find_iter /
// leftmost_find_iter (a batch: the CSR list, ends relative to the document).  Positions below are "absolute": bytes from the first byte
// of the text (a batch: of document 0), so the ends A_i of the matches are non-decreasing over the whole list and the documents begin at
// D_d = doc_off[d] - doc_off[0], D_n = len.  A single haystack is a batch of one document whose two offsets are {0, len}.
//
// Tokens come in two kinds.  A byte token begins at a byte p and is not empty: a non-empty match that starts at p, or a gap token.
// Byte p is "flagged" when one begins there, which is decided by the matches and documents that touch p and (DAAC_GAP_CHARS) hay[p]
// alone.  An empty-match token sits at a position, between bytes.  With rank(p) the number of flagged bytes before p and E_i the number
// of empty matches among matches [0, i), in the output
//     the byte token at p         has index rank(p) + E_c, c = the number of matches with A_i <= p,
//     the token of empty match i  has index rank(A_i) + E_i,
// and, for every gap rule but DAAC_GAP_SKIP, the byte tokens tile each document, so a gap token ends where the next flagged byte is, or
// at len: the next byte token (or position len) writes that end.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace daac {

constexpr uint32_t kTokLanes = 256;               // lanes of a workgroup, 16 bytes of text each
constexpr uint32_t kTokTile = kTokLanes * 16;     // bytes of text a workgroup reads per turn
constexpr uint32_t kTokMaxBlocks = 1u << 16;      // workgroups of the count and write passes; they stride over the tiles

struct TokenizeArgs {
    const uint8_t *hay;                    // byte 0 of the text (a batch: of document 0), any alignment
    uint64_t len;                          // bytes of text
    const uint4 *seg;                      // k tuples, as the tuple calls leave them
    uint64_t k;
    unsigned long long *aend;              // k: A_i
    unsigned long long *epre;              // k + 1: "match i is empty", then E_i (entry k: the number of empty matches)
    uint64_t n_empty;                      // known after the sum; 0 lets the write pass leave epre alone
    const unsigned long long *doc_first;   // a batch: n_docs + 1 CSR offsets of the tuple list; NULL: the ends are absolute already
    const unsigned long long *doc_off;     // n_docs + 1 (never NULL)
    uint64_t n_docs;                       // >= 1
    int gap;
    uint32_t gap_id;
    uint64_t tiles;                        // len / kTokTile + 1: position len has a lane of its own
    unsigned long long *tile_lo;           // tiles + 1: the number of matches with A_i < the tile's first byte (entry `tiles`: k)
    unsigned long long *tile_doc;          // tiles + 1: the number of d in [0, n_docs] with D_d < the tile's first byte (entry `tiles`: n_docs + 1)
    unsigned long long *tile_cnt;          // tiles + 1: flagged bytes of the tile, then their exclusive sum
    // the write pass
    uint32_t *ids;
    unsigned long long *spans;             // NULL: not wanted
    unsigned long long *tok_offsets;       // NULL: not wanted (a single haystack)
};

// one lane per match: A_i and the empty flag
hipError_t launch_tokenize_prep(const TokenizeArgs &a, hipStream_t stream);
// tile_lo and tile_doc (one lane per tile, a binary search each), then tile_cnt
hipError_t launch_tokenize_count(const TokenizeArgs &a, hipStream_t stream);
// ids, spans and tok_offsets, after the sums; nothing is stored at a token index of n_tokens or beyond
hipError_t launch_tokenize_write(const TokenizeArgs &a, uint64_t n_tokens, hipStream_t stream);

}  // namespace daac
