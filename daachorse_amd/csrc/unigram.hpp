// tokenize_unigram on the device (daac_tokenize_unigram, daac_tokenize_unigram_batch): what api_unigram.hip and unigram_kernels.hip share.
//
// The definition (include/daachorse_amd.h has it in full).  Every document is a problem of its own.  For a document of L bytes the nodes
// are the byte positions 0 .. L.  Every match (start, end, value) of find_overlapping_iter with start < end is an edge start -> end with
// score scores[value] and id value.  The cuts are 0, L and (DAAC_GAP_BYTES) every position, (DAAC_GAP_CHARS) every p whose byte is no
// UTF-8 continuation byte; consecutive cuts c -> c' are an "unknown" edge with score unk_score and id gap_id (_CHARS) or gap_id + doc[c]
// (_BYTES).  best[0] = +0.0f; for q = 1 .. L the incumbent starts at -inf with no edge, the candidates are the match edges into q in the
// order of the tuple list and then the unknown edge into q (if q is a cut), a candidate is the one float32 addition best[from] + score and
// replaces the incumbent only when strictly greater.  The tokens are the edges on the back-pointer path from L to 0, in text order, and
// the document's score is best[L].
//
// The input is the text and the CSR list of 16-byte tuples {end u64, length u32, value u32} of daac_scan_batch_device16
// (DAAC_FIND_OVERLAPPING): document d's tuples are [doc_first[d], doc_first[d+1]), ends relative to the document and non-decreasing.
// The unit of parallelism is the document: one lane walks one document.  Its scratch is a slice of two arrays of len + n positions
// (document d's position q is entry D_d + d + q, D_d = doc_off[d] - doc_off[0]): best (float) and the back pointer {edge length, id}.
//
// Limits: a wave takes as long as its longest document, and one long document (a single haystack is one) is walked by a single lane.
// A document of 2^32 - 1 bytes or more is refused (an edge's length is kept in 32 bits; it also bounds the number of additions of a path).
#pragma once

#include <cstdint>

#ifndef DAAC_UNIGRAM_HOST
#include <hip/hip_runtime.h>
#endif

namespace daac {

constexpr uint32_t kUniLanes = 256;           // lanes of a workgroup: 256 documents
constexpr uint32_t kUniMaxBlocks = 1u << 16;  // workgroups of a pass; they stride over the documents

struct alignas(16) UniTuple {   // daac_match16
    uint64_t end;
    uint32_t len;
    uint32_t value;
};
struct alignas(8) UniBack {     // the edge that won at a position
    uint32_t len;
    uint32_t id;
};

struct UnigramArgs {
    const uint8_t *hay;                    // byte 0 of document 0, any alignment
    const UniTuple *seg;                   // the tuple list
    const unsigned long long *doc_first;   // n_docs + 1 CSR offsets into seg
    const unsigned long long *doc_off;     // n_docs + 1 offsets of the documents (document d's bytes: hay + doc_off[d] - doc_off[0] ..)
    uint64_t n_docs;
    const float *scores;                   // n_scores, indexed by match value
    uint64_t n_scores;
    float unk_score;
    int gap;                               // DAAC_GAP_BYTES or DAAC_GAP_CHARS
    uint32_t gap_id;
    float *best;                           // len + n_docs positions
    UniBack *back;                         // len + n_docs positions (entry of a document's position 0: never read)
    float *doc_scores;                     // n_docs, or NULL: not wanted
    unsigned long long *tok_offsets;       // n_docs + 1: the token counts (entry n_docs: 0), then their exclusive sum
    // the write pass
    uint32_t *ids;
    unsigned long long *spans;             // NULL: not wanted
};

#ifndef DAAC_UNIGRAM_HOST
// one lane per document: best, back and doc_scores
hipError_t launch_unigram_forward(const UnigramArgs &a, hipStream_t stream);
// one lane per document: tok_offsets[d] = the number of edges on its path; tok_offsets[n_docs] = 0
hipError_t launch_unigram_count(const UnigramArgs &a, hipStream_t stream);
// ids and spans of every document, filled from the back of its range [tok_offsets[d], tok_offsets[d+1])
hipError_t launch_unigram_write(const UnigramArgs &a, hipStream_t stream);
#endif

}  // namespace daac
