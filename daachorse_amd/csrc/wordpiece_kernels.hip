// tokenize_wordpiece for gfx950 (daac_tokenize_wordpiece, daac_tokenize_wordpiece_batch): greedy longest-match-first with an initial and
// a continuation piece set over the tuple list of an overlapping scan.  wordpiece.hpp has the definition and the layout of the slots.
//
//   count  one lane per document.  It counts the document's characters (bytes that are no UTF-8 continuation byte) as far as max_chars,
//          clears its own L + 1 slots to "none", sweeps its tuples once into best[start] = {end, id} — a tuple whose id exists in the
//          role of its start replaces a shorter one — and walks p = 0 -> best[p].end -> .. to L.  The number of hops goes to
//          tok_offsets[d] and the verdict to the slot at L; a hop that finds nothing makes the document one unk_id token.  An exclusive
//          sum makes the counts offsets.
//   write  the lane reads the verdict, walks best[] again and fills its range of ids (and spans) in text order.
//
// Every word is written by the one lane that owns the document: vector stores, no atomics, no LDS.  Integer work only: the result is a
// function of the input alone.  Reads stay inside the document's bytes, its own tuple range [doc_first[d], doc_first[d+1]) and its own
// slots: a tuple whose fields do not fit the document (never produced) or whose value is beyond the id tables is ignored, and a link
// that does not advance or points beyond L (never produced) ends the walk as unk_id instead of leaving the slice.
//
// The per-lane bodies below are plain C++: with DAAC_WORDPIECE_HOST defined this file compiles without HIP and a host program runs them
// document by document (tests/native/wordpiece_check.cpp, under ASan and UBSan).
#ifndef DAAC_WORDPIECE_HOST
#include <hip/hip_runtime.h>
#define WP_FN static __device__ __forceinline__
#else
#define WP_FN static inline
#endif

#include <cstdint>

#include "wordpiece.hpp"

namespace daac {

struct WpDoc {             // what a lane knows of its document
    const uint8_t *text;   // its first byte
    uint32_t len;          // 0: nothing to do (empty, skipped, or too long for 32 bits)
    WpSlot *slot;          // its position 0
    const WpTuple *seg;    // its tuples
    uint64_t nt;
};

WP_FN WpDoc wp_doc(const WpArgs &a, uint64_t d) {
    WpDoc x;
    const uint64_t begin = a.doc_off[d] - a.doc_off[0];
    const uint64_t len = a.doc_off[d + 1] - a.doc_off[d];
    x.text = a.hay + begin;
    x.len = len < kWpMaxDoc && !(a.skip && a.skip[d]) ? static_cast<uint32_t>(len) : 0u;
    x.slot = a.slots + begin + d;
    const uint64_t t0 = a.doc_first[d], t1 = a.doc_first[d + 1];
    x.seg = a.seg + t0;
    x.nt = t1 <= t0 ? 0 : t1 - t0;
    return x;
}

// the characters, best[], the walk -> the number of tokens; the verdict goes to the slot at L
WP_FN uint64_t wp_count_lane(const WpArgs &a, uint64_t d) {
    const WpDoc x = wp_doc(a, d);
    const uint32_t L = x.len;
    if (!L) return 0;
    WpSlot *S = x.slot;
    uint64_t chars = 0;
    for (uint32_t q = 0; q < L && chars <= a.max_chars; ++q) chars += (x.text[q] & 0xC0u) != 0x80u;
    if (chars > a.max_chars) {   // too many characters: unk_id
        S[L] = WpSlot{0u, 0u};
        return 1;
    }
    for (uint32_t q = 0; q <= L; ++q) S[q] = WpSlot{0u, 0u};
    for (uint64_t t = 0; t < x.nt; ++t) {
        const WpTuple m = x.seg[t];
        if (m.len == 0 || m.end > L || m.len > m.end || m.value >= a.n_ids) continue;
        const uint32_t e = static_cast<uint32_t>(m.end), s = e - m.len;
        const uint32_t id = s ? a.cont_ids[m.value] : a.first_ids[m.value];
        if (id != kWpNone && e > S[s].end) S[s] = WpSlot{e, id};
    }
    uint64_t n = 0;
    for (uint32_t p = 0; p < L; ++n) {
        const uint32_t e = S[p].end;
        if (e <= p || e > L) return 1;   // no piece at p (or a link that leaves the document): unk_id; the verdict at L stays 0
        p = e;
    }
    S[L].id = 1u;
    return n;
}

WP_FN void wp_write_lane(const WpArgs &a, uint64_t d) {
    const uint64_t end = a.tok_offsets[d + 1];
    uint64_t idx = a.tok_offsets[d];
    if (idx >= end) return;   // empty, skipped
    const WpDoc x = wp_doc(a, d);
    const uint32_t L = x.len;
    if (!L) return;           // (never: such a document counted no token)
    if (x.slot[L].id != 1u) {
        a.ids[idx] = a.unk_id;
        if (a.spans) { a.spans[2 * idx] = 0; a.spans[2 * idx + 1] = L; }
        return;
    }
    for (uint32_t p = 0; p < L && idx < end; ++idx) {
        const WpSlot b = x.slot[p];
        if (b.end <= p || b.end > L) break;
        a.ids[idx] = b.id;
        if (a.spans) { a.spans[2 * idx] = p; a.spans[2 * idx + 1] = b.end; }
        p = b.end;
    }
}

#ifndef DAAC_WORDPIECE_HOST
// ------------------------------------------------------------------------------------------------------- kernels and launchers
__global__ __launch_bounds__(kWpLanes) void wordpiece_count_kernel(const WpArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride)
        a.tok_offsets[d] = d < a.n_docs ? wp_count_lane(a, d) : 0ull;   // (the sum's entry n_docs is the total)
}

__global__ __launch_bounds__(kWpLanes) void wordpiece_write_kernel(const WpArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d < a.n_docs; d += stride) wp_write_lane(a, d);
}

static uint32_t wp_grid(uint64_t docs) {
    const uint64_t g = (docs + kWpLanes - 1) / kWpLanes;
    return static_cast<uint32_t>(g < 1 ? 1 : g > kWpMaxBlocks ? kWpMaxBlocks : g);
}

hipError_t launch_wordpiece_count(const WpArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(wordpiece_count_kernel, dim3(wp_grid(a.n_docs + 1)), dim3(kWpLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_wordpiece_write(const WpArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(wordpiece_write_kernel, dim3(wp_grid(a.n_docs)), dim3(kWpLanes), 0, stream, a);
    return hipGetLastError();
}
#endif

}  // namespace daac
