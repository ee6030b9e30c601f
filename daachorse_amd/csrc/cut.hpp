// cut_batch and tokens_splice on the device (daac_cut_batch, daac_tokens_splice): what api_cut.hip and cut_kernels.hip share, and the
// per-lane bodies of the kernels.
//
// The definition (include/daachorse_amd.h has it in full).  Document i of a batch is cut at the matches of leftmost_find_iter on that
// document alone: every match is a *special* segment with the match's value, every non-empty stretch of text in front of the first
// match, between two matches and behind the last one is a *text* segment with the value kCutText.  tokens_splice takes what a
// tokenizer made of the segment batch and gives it back per document: a text segment's tokens are copied, a special segment is the one
// token {value, the segment}, and spans count from the document's first byte.
//
// The input of the cut is the CSR list of 16-byte tuples {end u64, length u32, value u32} of daac_scan_batch_device16
// (DAAC_LEFTMOST_FIND): document i's tuples are [doc_first[i], doc_first[i+1]), ends relative to the document, ascending, disjoint.
// The unit of parallelism is the *item*: in document order every document and behind it its matches, n_docs + k of them.  Document
// i's item is i + doc_first[i], its j-th match's item one more than that plus j.  An item finds its document by binary search over
// that strictly increasing function, so no lane walks a document's matches.  An item contributes
//   a document   1 segment when text stands in front of its first match, or when it has no match and is not empty
//   a match      1 for itself, and 1 more when text follows it before the next match or the document's end
// The counts are summed (one read-back of the total) and a second pass writes every item's segments at its rank; doc_segs[i] is the
// rank of document i's item.  Both passes decide an item's contribution with the same function, so the write pass stays inside the
// n_segs + 1 entries whatever the tuples hold.
//
// The splice counts a segment's output tokens (seg_tok[s+1] - seg_tok[s], or 1), sums them to the new per-segment token offsets, and
// a wave writes a segment with its lanes over the segment's tokens.  A segment finds its document by binary search in doc_segs.
//
// Integer work only, no atomics, no LDS: the result is a function of the input alone.  The per-lane bodies below are plain C++: with
// DAAC_CUT_HOST defined this file compiles without HIP and a host program runs them item by item (tests/native/cut_check.cpp).
#pragma once

#include <cstdint>

#ifndef DAAC_CUT_HOST
#include <hip/hip_runtime.h>
#define CUT_FN static __host__ __device__ __forceinline__
#else
#define CUT_FN static inline
#endif

namespace daac {

constexpr uint32_t kCutLanes = 256;            // lanes of a workgroup
constexpr uint32_t kCutMaxBlocks = 1u << 16;   // workgroups of a pass; they stride over the items
constexpr uint32_t kCutText = 0xFFFFFFFFu;     // the value of a text segment

struct alignas(16) CutTuple {   // daac_match16
    uint64_t end;
    uint32_t len;
    uint32_t value;
};

struct CutArgs {
    const CutTuple *seg;                   // the tuple list
    const unsigned long long *doc_first;   // n_docs + 1 CSR offsets into seg
    const unsigned long long *doc_off;     // n_docs + 1 offsets of the documents
    uint64_t n_docs;
    uint64_t k;                            // tuples: doc_first[n_docs]
    unsigned long long *counts;            // n_docs + k + 1: the items' contributions (the last entry: 0), then their exclusive sum
    // the write pass
    unsigned long long *seg_offsets;       // n_segs + 1
    unsigned long long *doc_segs;          // n_docs + 1
    uint32_t *seg_values;                  // n_segs
};

struct SpliceArgs {
    const uint32_t *ids;                     // the segment batch's tokens
    const unsigned long long *spans;         // NULL: not wanted
    const unsigned long long *seg_tok;       // n_segs + 1 token offsets of the segment batch
    const uint32_t *seg_values;              // n_segs
    const unsigned long long *seg_offsets;   // n_segs + 1
    const unsigned long long *doc_segs;      // n_docs + 1
    const unsigned long long *doc_off;       // n_docs + 1
    uint64_t n_segs, n_docs;
    unsigned long long *out_seg_tok;         // n_segs + 1: the output counts (the last entry: 0), then their exclusive sum
    // the write pass
    uint32_t *out_ids;
    unsigned long long *out_spans;           // NULL: not wanted
};

// the largest i in [0, n) with key(i) <= x, for a non-decreasing key with key(0) <= x
template <class Key>
CUT_FN uint64_t cut_last_le(uint64_t n, uint64_t x, Key key) {
    uint64_t lo = 0, hi = n;   // key(lo) <= x, key(hi) > x (hi == n: none)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (key(mid) <= x) lo = mid; else hi = mid;
    }
    return lo;
}

struct CutItem {     // what a lane knows of its item
    uint64_t doc;    // its document
    uint64_t base;   // the document's first byte
    uint64_t len;    // the document's bytes
    bool is_doc;
    uint64_t start, end;   // a match: its bytes, relative to the document and inside it; a document: start = the first match's start, or len
    uint32_t value;
    uint64_t next;   // a match: where the next match starts, or len
};

// a tuple's bytes, kept inside [floor, len] (a tuple that does not fit its document is never produced)
CUT_FN void cut_clip(const CutTuple &m, uint64_t floor, uint64_t len, uint64_t &s, uint64_t &e) {
    e = m.end > len ? len : m.end;
    s = m.len > e ? 0 : e - m.len;
    if (s < floor) s = floor;
    if (e < s) e = s;
}

CUT_FN CutItem cut_item(const CutArgs &a, uint64_t x) {
    CutItem it;
    const unsigned long long *df = a.doc_first;
    it.doc = cut_last_le(a.n_docs, x, [df](uint64_t i) { return i + df[i]; });
    const uint64_t t0 = df[it.doc], t1 = df[it.doc + 1];
    it.base = a.doc_off[it.doc];
    it.len = a.doc_off[it.doc + 1] - it.base;
    it.is_doc = x == it.doc + t0;
    it.value = kCutText;
    uint64_t s, e;
    if (it.is_doc) {
        it.start = it.len;
        if (t1 > t0) { cut_clip(a.seg[t0], 0, it.len, s, e); it.start = s; }
        it.end = it.next = it.start;
        return it;
    }
    const uint64_t t = t0 + (x - it.doc - t0 - 1);
    const CutTuple m = a.seg[t];
    uint64_t floor = 0;
    if (t > t0) { cut_clip(a.seg[t - 1], 0, it.len, s, e); floor = e; }
    cut_clip(m, floor, it.len, it.start, it.end);
    it.value = m.value;
    it.next = it.len;
    if (t + 1 < t1) { cut_clip(a.seg[t + 1], it.end, it.len, s, e); it.next = s; }
    return it;
}

CUT_FN uint64_t cut_contribution(const CutItem &it) {
    if (it.is_doc) return it.start > 0 ? 1 : 0;
    return 1 + (it.next > it.end ? 1 : 0);
}

// item x of n_docs + k; x == n_docs + k is the closing entry
CUT_FN uint64_t cut_count_lane(const CutArgs &a, uint64_t x) {
    return x < a.n_docs + a.k ? cut_contribution(cut_item(a, x)) : 0;
}

CUT_FN void cut_write_lane(const CutArgs &a, uint64_t x) {
    const uint64_t r = a.counts[x];
    if (x >= a.n_docs + a.k) {   // the closing entries
        a.seg_offsets[r] = a.doc_off[a.n_docs];
        a.doc_segs[a.n_docs] = r;
        return;
    }
    const CutItem it = cut_item(a, x);
    if (it.is_doc) {
        a.doc_segs[it.doc] = r;
        if (it.start > 0) { a.seg_offsets[r] = it.base; a.seg_values[r] = kCutText; }
        return;
    }
    a.seg_offsets[r] = it.base + it.start;
    a.seg_values[r] = it.value;
    if (it.next > it.end) { a.seg_offsets[r + 1] = it.base + it.end; a.seg_values[r + 1] = kCutText; }
}

// ---- the splice
CUT_FN uint64_t splice_seg_tokens(const SpliceArgs &a, uint64_t s) {
    const uint64_t t0 = a.seg_tok[s], t1 = a.seg_tok[s + 1];
    return t1 > t0 ? t1 - t0 : 0;
}

CUT_FN uint64_t splice_count_lane(const SpliceArgs &a, uint64_t s) {
    if (s >= a.n_segs) return 0;
    return a.seg_values[s] == kCutText ? splice_seg_tokens(a, s) : 1;
}

// segment s, the tokens lane, lane + lanes, .. of it
CUT_FN void splice_write_segment(const SpliceArgs &a, uint64_t s, uint32_t lane, uint32_t lanes) {
    const uint64_t o = a.out_seg_tok[s];
    const uint32_t value = a.seg_values[s];
    uint64_t delta = 0;
    if (a.out_spans) {
        const unsigned long long *ds = a.doc_segs;
        const uint64_t d = cut_last_le(a.n_docs, s, [ds](uint64_t i) { return static_cast<uint64_t>(ds[i]); });
        delta = a.seg_offsets[s] - a.doc_off[d];
    }
    if (value != kCutText) {
        if (lane != 0) return;
        a.out_ids[o] = value;
        if (a.out_spans) { a.out_spans[2 * o] = delta; a.out_spans[2 * o + 1] = delta + (a.seg_offsets[s + 1] - a.seg_offsets[s]); }
        return;
    }
    const uint64_t n = splice_seg_tokens(a, s), t0 = a.seg_tok[s];
    for (uint64_t t = lane; t < n; t += lanes) {
        a.out_ids[o + t] = a.ids[t0 + t];
        if (a.out_spans) {
            a.out_spans[2 * (o + t)] = a.spans[2 * (t0 + t)] + delta;
            a.out_spans[2 * (o + t) + 1] = a.spans[2 * (t0 + t) + 1] + delta;
        }
    }
}

#ifndef DAAC_CUT_HOST
// counts[x] for the n_docs + k items and the closing 0
hipError_t launch_cut_count(const CutArgs &a, hipStream_t stream);
// seg_offsets, seg_values and doc_segs, the closing entries included, from the summed counts
hipError_t launch_cut_write(const CutArgs &a, hipStream_t stream);
// out_seg_tok[s] for the n_segs segments and the closing 0
hipError_t launch_splice_count(const SpliceArgs &a, hipStream_t stream);
// out_ids and out_spans from the summed out_seg_tok: a wave a segment
hipError_t launch_splice_write(const SpliceArgs &a, hipStream_t stream);
#endif

}  // namespace daac
