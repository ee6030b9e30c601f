// tokenize_bpe on the device (daac_tokenize_bpe, daac_tokenize_bpe_batch): what api_bpe.hip and bpe_kernels.hip share.
//
// The definition (include/daachorse_amd.h has it in full).  Every document is a problem of its own.  For a document doc of L bytes,
// piece(s, e) for 0 <= s < e <= L is the value v of the match (s, e, v) of find_overlapping_iter(doc), absent when there is none, and
// rank(s, e) is ranks[v] (no table: v); a rank of 0xFFFFFFFF is never the product of a merge.  The initial boundaries are 0, L and
// (DAAC_GAP_BYTES) every position, (DAAC_GAP_CHARS) every p whose byte is no UTF-8 continuation byte.  With the live boundaries
// p_0 = 0 < p_1 < .. < p_k = L, the merge loop takes among all i whose piece(p_i, p_{i+2}) is present with a rank below 0xFFFFFFFF the one
// of smallest rank, on ties the smallest i, removes p_{i+1}, and repeats until there is no such i.  A final part (p_i, p_{i+1}) is one
// token: its id is piece(p_i, p_{i+1}) when present, otherwise (an initial part the vocabulary lacks) gap_id + doc[p_i] (_BYTES) or
// gap_id (_CHARS).
//
// The input is the text and the CSR list of 16-byte tuples {end u64, length u32, value u32} of daac_scan_batch_device16
// (DAAC_FIND_OVERLAPPING): document d's tuples are [doc_first[d], doc_first[d+1]), ends relative to the document and non-decreasing.
// The unit of parallelism is the document: one lane walks one document.  Its scratch is a slice of one array of len + n slots (document
// d's position q is entry D_d + d + q, D_d = doc_off[d] - doc_off[0]; positions 0 .. L), 24 bytes a slot:
//   next  the live boundary after q; 0 at L (a boundary only; a link of 0, one that does not advance or one beyond L ends a walk)
//   rank  the rank of the pair of parts that begins at q, piece(q, next[next[q]]); 0xFFFFFFFF: absent, or never merged (next and
//         rank are what the minimum scan reads: one 8-byte load)
//   id    the token id of the part that begins at q
//   val   the value of that pair, which becomes id[q] when the pair is merged
//   prev  the live boundary before q (a boundary other than 0 only)
//   tix   the first tuple of the document with end >= q, counted from doc_first[d] (every position; the document's tuple count if none)
// A document has fewer than 2^32 tuples: it is at most 65536 bytes (option bpe_doc_max) and an end has at most one tuple per start and
// one empty match.  A lane looks at no more than the first 2^32 - 1 tuples of its range.
//
// Limits: the merge loop scans a document's live parts once per merge, up to L^2 / 2 part visits on one lane, so a document longer
// than option bpe_doc_max (4096; 1 .. 65536) is refused before a kernel of this file is launched.
#pragma once

#include <cstdint>

#ifndef DAAC_BPE_HOST
#include <hip/hip_runtime.h>
#endif

namespace daac {

constexpr uint32_t kBpeLanes = 256;           // lanes of a workgroup: 256 documents
constexpr uint32_t kBpeMaxBlocks = 1u << 16;  // workgroups of a pass; they stride over the documents
constexpr uint32_t kBpeNoRank = 0xFFFFFFFFu;  // the rank that is never merged
constexpr uint64_t kBpeDocCap = 65536;        // the largest bpe_doc_max

struct alignas(16) BpeTuple {   // daac_match16
    uint64_t end;
    uint32_t len;
    uint32_t value;
};
struct alignas(8) BpeSlot {     // one position of a document (see above)
    uint32_t next, rank, id, val, prev, tix;
};
static_assert(sizeof(BpeSlot) == 24, "24 bytes a slot");

struct BpeArgs {
    const uint8_t *hay;                    // byte 0 of document 0, any alignment
    const BpeTuple *seg;                   // the tuple list
    const unsigned long long *doc_first;   // n_docs + 1 CSR offsets into seg
    const unsigned long long *doc_off;     // n_docs + 1 offsets of the documents (document d's bytes: hay + doc_off[d] - doc_off[0] ..)
    uint64_t n_docs;
    const uint32_t *ranks;                 // n_ranks, indexed by match value; NULL: a piece's rank is its value
    uint64_t n_ranks;
    uint64_t doc_max;                      // a longer document is left alone (the driver has refused it)
    int gap;                               // DAAC_GAP_BYTES or DAAC_GAP_CHARS
    uint32_t gap_id;
    BpeSlot *slots;                        // len + n_docs positions
    unsigned long long *tok_offsets;       // n_docs + 1: the token counts (entry n_docs: 0), then their exclusive sum
    // the write pass
    uint32_t *ids;
    unsigned long long *spans;             // NULL: not wanted
};

#ifndef DAAC_BPE_HOST
// one lane per document: the index, the merge loop, tok_offsets[d] = its live parts; tok_offsets[n_docs] = 0
hipError_t launch_bpe_merge(const BpeArgs &a, hipStream_t stream);
// ids and spans of every document, its range [tok_offsets[d], tok_offsets[d+1]) filled in text order
hipError_t launch_bpe_write(const BpeArgs &a, hipStream_t stream);
#endif

}  // namespace daac
