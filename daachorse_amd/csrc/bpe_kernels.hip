// tokenize_bpe for gfx950 (daac_tokenize_bpe, daac_tokenize_bpe_batch): byte-pair merging over the tuple list of an overlapping scan.
// bpe.hpp has the definition and the layout of the scratch slots.
//
//   merge  one lane per document.  index: it walks its tuples once and stores for every q = 0 .. L the first tuple with end >= q, so
//          piece(s, e) is a look through the tuples that end at e for the one of length e - s (as many candidates as patterns are
//          suffixes of one another there).  Then it links the initial boundaries, gives every initial part its id and every pair of
//          neighbours its cached rank and value, and loops: a linear minimum over the live pairs (strictly smaller wins, so ties go
//          left), unlink the boundary in the middle, recompute the two pairs that changed — tiktoken's byte_pair_merge for small
//          pieces.  The number of live parts goes to tok_offsets[d]; an exclusive sum makes them offsets.
//   write  the lane walks its boundary links from 0 and fills its range of ids (and spans) in text order.
//
// Every word is written by the one lane that owns the document: vector stores, no atomics, no LDS.  Integer work only: the result is a
// function of the input alone.  Reads stay inside the document's bytes, its own tuple range [doc_first[d], doc_first[d+1]) and its own
// slots: a tuple whose fields do not fit the document (never produced) matches no (s, e) that is asked for, and a link that is 0, does
// not advance or points beyond L (never produced) ends a walk instead of leaving the slice.
//
// The per-lane bodies below are plain C++: with DAAC_BPE_HOST defined this file compiles without HIP and a host program runs them
// document by document (tests/native/bpe_check.cpp, under ASan and UBSan).
#ifndef DAAC_BPE_HOST
#include <hip/hip_runtime.h>
#define BPE_FN static __device__ __forceinline__
#else
#define BPE_FN static inline
#endif

#include <cstdint>

#include "bpe.hpp"
#include "../../include/daachorse_amd.h"

namespace daac {

struct BpeDoc {            // what a lane knows of its document
    const uint8_t *text;   // its first byte
    uint32_t len;          // 0: nothing to do (empty, or longer than doc_max)
    BpeSlot *slot;         // its position 0
    const BpeTuple *seg;   // its tuples
    uint32_t nt;
};

BPE_FN BpeDoc bpe_doc(const BpeArgs &a, uint64_t d) {
    BpeDoc x;
    const uint64_t begin = a.doc_off[d] - a.doc_off[0];
    const uint64_t len = a.doc_off[d + 1] - a.doc_off[d];
    x.text = a.hay + begin;
    x.len = len <= a.doc_max && len <= kBpeDocCap ? static_cast<uint32_t>(len) : 0u;
    x.slot = a.slots + begin + d;
    const uint64_t t0 = a.doc_first[d], t1 = a.doc_first[d + 1];
    x.seg = a.seg + t0;
    x.nt = t1 <= t0 ? 0u : t1 - t0 < 0xFFFFFFFFull ? static_cast<uint32_t>(t1 - t0) : 0xFFFFFFFFu;
    return x;
}

// piece(s, e) for 0 <= s < e <= L (a tuple of length 0, or longer than its end, equals no e - s)
BPE_FN bool bpe_piece(const BpeDoc &x, uint32_t s, uint32_t e, uint32_t &value) {
    for (uint32_t t = x.slot[e].tix; t < x.nt; ++t) {
        const BpeTuple m = x.seg[t];
        if (m.end != e) break;
        if (m.len == e - s) { value = m.value; return true; }
    }
    return false;
}

BPE_FN uint32_t bpe_rank(const BpeArgs &a, uint32_t value) {
    if (!a.ranks) return value;
    return value < a.n_ranks ? a.ranks[value] : kBpeNoRank;   // (the driver has checked n_ranks against the largest value)
}

// the cached rank and value of the pair of parts that begins at boundary p < L
BPE_FN void bpe_pair(const BpeArgs &a, const BpeDoc &x, uint32_t p) {
    uint32_t rank = kBpeNoRank, val = 0;
    const uint32_t n = x.slot[p].next;
    if (n > p && n < x.len) {
        const uint32_t nn = x.slot[n].next;
        uint32_t v;
        if (nn > n && nn <= x.len && bpe_piece(x, p, nn, v)) { rank = bpe_rank(a, v); val = v; }
    }
    x.slot[p].rank = rank;
    x.slot[p].val = val;
}

// index, initial parts, merge loop -> the number of final parts
BPE_FN uint64_t bpe_merge_lane(const BpeArgs &a, uint64_t d) {
    const BpeDoc x = bpe_doc(a, d);
    const uint32_t L = x.len;
    if (!L) return 0;
    BpeSlot *S = x.slot;
    for (uint32_t q = 0, t = 0; q <= L; ++q) {          // index: the tuples' ends do not decrease
        while (t < x.nt && x.seg[t].end < q) ++t;
        S[q].tix = t;
    }
    uint32_t parts = 0, b = 0, b_byte = x.text[0];       // the boundary before q and the byte there
    for (uint32_t q = 1; q <= L; ++q) {
        const uint32_t byte = q < L ? x.text[q] : 0u;
        if (q != L && a.gap != DAAC_GAP_BYTES && (byte & 0xC0u) == 0x80u) continue;
        uint32_t v;
        S[b].id = bpe_piece(x, b, q, v) ? v : a.gap_id + (a.gap == DAAC_GAP_BYTES ? b_byte : 0u);
        S[b].next = q;
        S[q].prev = b;
        b = q;
        b_byte = byte;
        ++parts;
    }
    S[0].prev = 0;
    S[L].next = 0;
    S[L].id = 0;
    S[L].rank = kBpeNoRank;
    S[L].val = 0;
    for (uint32_t p = 0; p < L;) {
        bpe_pair(a, x, p);
        const uint32_t n = S[p].next;
        if (n <= p) break;
        p = n;
    }
    for (uint32_t round = 1; round < L; ++round) {        // a merge takes a boundary away: fewer than L of them
        uint32_t best = kBpeNoRank, at = 0;
        for (uint32_t p = 0; p < L;) {
            const uint32_t r = S[p].rank, n = S[p].next;
            if (r < best) { best = r; at = p; }
            if (n <= p) break;
            p = n;
        }
        if (best == kBpeNoRank) break;
        const uint32_t m = S[at].next;
        if (m <= at || m >= L) break;                     // (never: a cached rank stands at a pair)
        const uint32_t nn = S[m].next;
        if (nn <= m || nn > L) break;
        S[at].id = S[at].val;
        S[at].next = nn;
        S[nn].prev = at;
        --parts;
        bpe_pair(a, x, at);
        if (at) {
            const uint32_t pv = S[at].prev;
            if (pv < at) bpe_pair(a, x, pv);
        }
    }
    return parts;
}

BPE_FN void bpe_write_lane(const BpeArgs &a, uint64_t d) {
    const BpeDoc x = bpe_doc(a, d);
    const uint64_t end = a.tok_offsets[d + 1];
    uint64_t idx = a.tok_offsets[d];
    for (uint32_t p = 0; p < x.len && idx < end; ++idx) {
        const uint32_t n = x.slot[p].next;
        if (n <= p || n > x.len) break;
        a.ids[idx] = x.slot[p].id;
        if (a.spans) { a.spans[2 * idx] = p; a.spans[2 * idx + 1] = n; }
        p = n;
    }
}

#ifndef DAAC_BPE_HOST
// ------------------------------------------------------------------------------------------------------- kernels and launchers
__global__ __launch_bounds__(kBpeLanes) void bpe_merge_kernel(const BpeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride)
        a.tok_offsets[d] = d < a.n_docs ? bpe_merge_lane(a, d) : 0ull;   // (the sum's entry n_docs is the total)
}

__global__ __launch_bounds__(kBpeLanes) void bpe_write_kernel(const BpeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d < a.n_docs; d += stride) bpe_write_lane(a, d);
}

static uint32_t bpe_grid(uint64_t docs) {
    const uint64_t g = (docs + kBpeLanes - 1) / kBpeLanes;
    return static_cast<uint32_t>(g < 1 ? 1 : g > kBpeMaxBlocks ? kBpeMaxBlocks : g);
}

hipError_t launch_bpe_merge(const BpeArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(bpe_merge_kernel, dim3(bpe_grid(a.n_docs + 1)), dim3(kBpeLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_bpe_write(const BpeArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(bpe_write_kernel, dim3(bpe_grid(a.n_docs)), dim3(kBpeLanes), 0, stream, a);
    return hipGetLastError();
}
#endif

}  // namespace daac
