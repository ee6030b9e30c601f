// tokenize_unigram for gfx950 (daac_tokenize_unigram, daac_tokenize_unigram_batch): the Viterbi pass over the tuple list of an
// overlapping scan.  unigram.hpp has the definition and the layout of the scratch arrays.
//
//   forward  one lane per document: walks q = 1 .. L, advancing through the document's tuples (their ends do not decrease), keeps the
//            previous cut as it reads the text, stores best[q] and the winning edge {length, id} of every position, then doc_scores[d].
//   count    the lane follows the back pointers from L and stores the number of edges; an exclusive sum makes them tok_offsets.
//   write    the lane follows them again and fills its range of ids (and spans) from the back.
//
// Every word is written by the one lane that owns the document: vector stores, no atomics, no LDS.  A candidate is one float32 addition
// (no multiply next to it, so nothing can be fused) compared with `>`, in the order of the definition: the result, score bits included,
// is a function of the input alone.  Reads stay inside the document's bytes, its own tuple range [doc_first[d], doc_first[d+1]) and its own
// slice of best / back: a tuple whose fields do not fit the document (never produced) is passed over, not followed.
//
// The three per-lane bodies below are plain C++: with DAAC_UNIGRAM_HOST defined this file compiles without HIP and a host program runs
// them document by document (tests/native/unigram_check.cpp, under ASan and UBSan).
#ifndef DAAC_UNIGRAM_HOST
#include <hip/hip_runtime.h>
#define UNI_FN static __device__ __forceinline__
#else
#define UNI_FN static inline
#endif

#include <cstdint>

#include "unigram.hpp"
#include "../../include/daachorse_amd.h"

namespace daac {

struct UniDoc {          // what a lane knows of its document
    const uint8_t *text; // its first byte
    uint64_t len;
    uint64_t slot;       // its position 0 in best / back
    uint64_t t0, t1;     // its tuples
};

UNI_FN UniDoc uni_doc(const UnigramArgs &a, uint64_t d) {
    UniDoc x;
    const uint64_t begin = a.doc_off[d] - a.doc_off[0];
    x.text = a.hay + begin;
    x.len = a.doc_off[d + 1] - a.doc_off[d];
    x.slot = begin + d;
    x.t0 = a.doc_first[d];
    x.t1 = a.doc_first[d + 1];
    return x;
}

UNI_FN void unigram_forward_lane(const UnigramArgs &a, uint64_t d) {
    const UniDoc x = uni_doc(a, d);
    const float ninf = -__builtin_huge_valf();
    float *best = a.best + x.slot;
    UniBack *back = a.back + x.slot;
    best[0] = 0.0f;
    uint64_t t = x.t0;
    uint64_t cut = 0;                                   // the previous cut
    uint32_t cut_byte = x.len ? x.text[0] : 0u;         // ... and the byte there
    float last = 0.0f;
    for (uint64_t q = 1; q <= x.len; ++q) {
        float inc = ninf;
        UniBack e{0u, 0u};
        for (; t < x.t1; ++t) {                         // the match edges into q, in the list's order
            const UniTuple m = a.seg[t];
            if (m.end > q) break;
            if (m.end < q || m.len == 0 || m.len > q || m.value >= a.n_scores) continue;   // "" at 0; the rest: never produced
            const float c = best[q - m.len] + a.scores[m.value];   // (-inf + score = -inf: an unreachable start never wins)
            if (c > inc) { inc = c; e.len = m.len; e.id = m.value; }
        }
        const uint32_t byte = q < x.len ? x.text[q] : 0u;
        if (q == x.len || a.gap == DAAC_GAP_BYTES || (byte & 0xC0u) != 0x80u) {   // q is a cut: the unknown edge cut -> q
            const float c = best[cut] + a.unk_score;
            if (c > inc) { inc = c; e.len = static_cast<uint32_t>(q - cut); e.id = a.gap_id + (a.gap == DAAC_GAP_BYTES ? cut_byte : 0u); }
            cut = q;
            cut_byte = byte;
        }
        best[q] = inc;
        back[q] = e;
        last = inc;
    }
    if (a.doc_scores) a.doc_scores[d] = last;
}

// The path from L to 0.  An edge of length 0 or beyond the position stands at no reachable node (every node of the path is reachable and
// L always is): the walk ends there instead of leaving the slice.
UNI_FN uint64_t unigram_count_lane(const UnigramArgs &a, uint64_t d) {
    const UniDoc x = uni_doc(a, d);
    const UniBack *back = a.back + x.slot;
    uint64_t cnt = 0;
    for (uint64_t q = x.len; q > 0; ++cnt) {
        const uint32_t l = back[q].len;
        if (l == 0 || l > q) break;
        q -= l;
    }
    return cnt;
}

UNI_FN void unigram_write_lane(const UnigramArgs &a, uint64_t d) {
    const UniDoc x = uni_doc(a, d);
    const UniBack *back = a.back + x.slot;
    const uint64_t first = a.tok_offsets[d];
    uint64_t idx = a.tok_offsets[d + 1];
    for (uint64_t q = x.len; q > 0 && idx > first;) {
        const UniBack e = back[q];
        if (e.len == 0 || e.len > q) break;
        --idx;
        a.ids[idx] = e.id;
        if (a.spans) { a.spans[2 * idx] = q - e.len; a.spans[2 * idx + 1] = q; }
        q -= e.len;
    }
}

#ifndef DAAC_UNIGRAM_HOST
// ------------------------------------------------------------------------------------------------------- kernels and launchers
__global__ __launch_bounds__(kUniLanes) void unigram_forward_kernel(const UnigramArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d < a.n_docs; d += stride) unigram_forward_lane(a, d);
}

__global__ __launch_bounds__(kUniLanes) void unigram_count_kernel(const UnigramArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride)
        a.tok_offsets[d] = d < a.n_docs ? unigram_count_lane(a, d) : 0ull;   // (the sum's entry n_docs is the total)
}

__global__ __launch_bounds__(kUniLanes) void unigram_write_kernel(const UnigramArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d < a.n_docs; d += stride) unigram_write_lane(a, d);
}

static uint32_t uni_grid(uint64_t docs) {
    const uint64_t g = (docs + kUniLanes - 1) / kUniLanes;
    return static_cast<uint32_t>(g < 1 ? 1 : g > kUniMaxBlocks ? kUniMaxBlocks : g);
}

hipError_t launch_unigram_forward(const UnigramArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(unigram_forward_kernel, dim3(uni_grid(a.n_docs)), dim3(kUniLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_unigram_count(const UnigramArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(unigram_count_kernel, dim3(uni_grid(a.n_docs + 1)), dim3(kUniLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_unigram_write(const UnigramArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(unigram_write_kernel, dim3(uni_grid(a.n_docs)), dim3(kUniLanes), 0, stream, a);
    return hipGetLastError();
}
#endif

}  // namespace daac
