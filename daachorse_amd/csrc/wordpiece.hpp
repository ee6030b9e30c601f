// tokenize_wordpiece on the device (daac_tokenize_wordpiece, daac_tokenize_wordpiece_batch): what api_wordpiece.hip and
// wordpiece_kernels.hip share.
//
// The definition (include/daachorse_amd.h has it in full).  Every document is a word, a problem of its own.  For a document of L bytes,
// piece(s, e) for 0 <= s < e <= L is the value v of the match (s, e, v) of find_overlapping_iter(doc); its id is first_ids[v] when
// s == 0 and cont_ids[v] otherwise, and a piece whose id is 0xFFFFFFFF does not exist in that role.  From p = 0 the longest piece that
// exists at p in its role is taken, until p == L; a p < L without a piece makes the whole document the one token {unk_id, 0, L}, and so
// does a document of more than max_chars bytes that are no UTF-8 continuation bytes.  An empty or a skipped document has no tokens.
//
// The input is the text and the CSR list of 16-byte tuples {end u64, length u32, value u32} of daac_scan_batch_device16
// (DAAC_FIND_OVERLAPPING): document d's tuples are [doc_first[d], doc_first[d+1]).  The unit of parallelism is the document: one lane
// walks one document.  Its scratch is a slice of one array of len + n slots (document d's position q is entry D_d + d + q,
// D_d = doc_off[d] - doc_off[0]; positions 0 .. L), 8 bytes a slot:
//   end   the end of the longest piece that exists in its role at start q; 0: none (a piece ends behind its start, so never at 0)
//   id    that piece's id.  At position L, where no piece starts, the verdict of the count pass: 1 = segmented, 0 = the one unk_id token
// A tuple is kept when its end is larger than the one the slot holds, so the result does not depend on the order of the tuples.  The
// work of a document is L + its tuples: there is no cap on a document below the 2^32 - 1 bytes that the 32-bit fields hold.
#pragma once

#include <cstdint>

#ifndef DAAC_WORDPIECE_HOST
#include <hip/hip_runtime.h>
#endif

namespace daac {

constexpr uint32_t kWpLanes = 256;            // lanes of a workgroup: 256 documents
constexpr uint32_t kWpMaxBlocks = 1u << 16;   // workgroups of a pass; they stride over the documents
constexpr uint32_t kWpNone = 0xFFFFFFFFu;     // in first_ids / cont_ids: no such piece
constexpr uint64_t kWpMaxDoc = 0xFFFFFFFFull; // a document has fewer bytes than this (the driver refuses the others)

struct alignas(16) WpTuple {   // daac_match16
    uint64_t end;
    uint32_t len;
    uint32_t value;
};
struct alignas(8) WpSlot {     // one position of a document (see above)
    uint32_t end, id;
};
static_assert(sizeof(WpSlot) == 8, "8 bytes a slot");

struct WpArgs {
    const uint8_t *hay;                    // byte 0 of document 0, any alignment
    const WpTuple *seg;                    // the tuple list
    const unsigned long long *doc_first;   // n_docs + 1 CSR offsets into seg
    const unsigned long long *doc_off;     // n_docs + 1 offsets of the documents (document d's bytes: hay + doc_off[d] - doc_off[0] ..)
    uint64_t n_docs;
    const uint32_t *first_ids;             // n_ids each, indexed by match value; kWpNone: no such piece
    const uint32_t *cont_ids;
    uint64_t n_ids;
    uint32_t unk_id;
    uint32_t max_chars;
    const uint8_t *skip;                   // NULL, or n_docs bytes: non-zero, the document yields no tokens
    WpSlot *slots;                         // len + n_docs positions
    unsigned long long *tok_offsets;       // n_docs + 1: the token counts (entry n_docs: 0), then their exclusive sum
    // the write pass
    uint32_t *ids;
    unsigned long long *spans;             // NULL: not wanted
};

#ifndef DAAC_WORDPIECE_HOST
// one lane per document: best[] from its tuples, the walk, tok_offsets[d] = its tokens and the verdict; tok_offsets[n_docs] = 0
hipError_t launch_wordpiece_count(const WpArgs &a, hipStream_t stream);
// ids and spans of every document, its range [tok_offsets[d], tok_offsets[d+1]) filled in text order
hipError_t launch_wordpiece_write(const WpArgs &a, hipStream_t stream);
#endif

}  // namespace daac
