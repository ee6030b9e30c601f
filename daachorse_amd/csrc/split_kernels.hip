// split_batch for gfx950 (daac_split_batch, daac_split, daac_offsets_compose): the word starts of a batch of documents as a streaming
// pass with one lane per byte, a bit mask and a compaction.  split.hpp has the scratch layout, include/daachorse_amd.h the definition.
//
//   marks    one lane per document: a non-empty document sets the bit of its first position (an empty one shares the bit of the
//            document behind it), the lane behind the last document sets bit `total`.  Device-scope atomicOr on 32-bit words.
//   flags    a workgroup takes a tile of kSplitTile positions.  It stages the tile's bytes with kSplitBack bytes in front and
//            kSplitAhead - 1 behind, and the tile's mark bits with a word on either side, in LDS.  A lane takes a position: the mark
//            bits around it say how many of the staged bytes belong to its document (split_reach), and split_start decides from
//            those bytes alone whether a word starts there.  One wave ballot makes one 64-bit word of the mask; the set bits of the
//            tile go to counts[tile], whose exclusive sum ranks the word starts.
//   scatter  rank = counts[tile] + the set bits of the tile's earlier mask words + those below the lane's bit; word_offsets[rank] =
//            base + position.  One lane per document looks up the rank of its first position the same way: doc_words.
//
// The local form of the rules that split_start evaluates, over the units u[i] of a document of n units and their classes c[i]:
//   AS(i): u[i] is ' and (i == 0, or c[i-1] is L or N, or c[i-1] is S and u[i-1] is not 0x20).
//   K(i):  0 unless AS(i); 2 if the bytes at i are 's 't 'm 'd; 3 if they are 're 've 'll; else 0.
//   start(0) is true; for i > 0 the first case that applies decides:
//     1. c[i] is S and c[i-1] is S: start iff i + 1 < n and c[i+1] is not S
//     2. c[i] is S: start                     3. c[i-1] is S: start iff u[i-1] is not 0x20
//     4. c[i] is L and (K(i-1) != 0 or K(i-2) == 3): no start
//     5. K(i-2) == 2 or K(i-3) == 3: start   6. otherwise: start iff c[i] != c[i-1]
//   DAAC_SPLIT_WHITESPACE: start(i) iff (c[i] is S) != (c[i-1] is S).
// A contraction is ASCII, so K is looked up by bytes: the farthest byte read is the unit in front of a ' three bytes back (7 bytes),
// the farthest ahead the unit behind a whitespace unit (4 + 4 bytes).
//
// Reads stay inside [offsets[0], offsets[n]): a staged byte outside it is 0 and no decision reads it, because position 0 and position
// `total` carry marks.  Writes: masks and counts by the lane that owns them, word_offsets[rank] guarded by the total.
//
// The per-position functions below are plain C++: with DAAC_SPLIT_HOST defined this file compiles without HIP and a host program
// evaluates them at every position of documents held in buffers of exactly their size (tests/native/split_check.cpp, under ASan and
// UBSan).
#ifndef DAAC_SPLIT_HOST
#include <hip/hip_runtime.h>
#define SPLIT_FN static __device__ __forceinline__
#else
#define SPLIT_FN static inline
#endif

#include <cstdint>

#include "split.hpp"
#include "../../include/daachorse_amd.h"

namespace daac {

// The bytes of the unit that begins at q, of whose document `avail` >= 1 bytes from q on may be read: 2 .. 4 for a well-formed
// sequence (Unicode Table 3-7) that fits, else 1.
SPLIT_FN int split_unit_len(const uint8_t *q, int avail) {
    const uint32_t b0 = q[0];
    if (b0 < 0xC2u || b0 > 0xF4u) return 1;
    int need;
    uint32_t lo = 0x80u, hi = 0xBFu;
    if (b0 < 0xE0u) need = 2;
    else if (b0 < 0xF0u) { need = 3; if (b0 == 0xE0u) lo = 0xA0u; if (b0 == 0xEDu) hi = 0x9Fu; }
    else { need = 4; if (b0 == 0xF0u) lo = 0x90u; if (b0 == 0xF4u) hi = 0x8Fu; }
    if (avail < need) return 1;
    if (q[1] < lo || q[1] > hi) return 1;
    for (int k = 2; k < need; ++k)
        if ((q[k] & 0xC0u) != 0x80u) return 1;
    return need;
}

// The bytes of the unit that ends in front of the unit start s, of whose document `before` >= 1 bytes in front of s may be read
// (all of them when fewer than 4).
SPLIT_FN int split_prev_len(const uint8_t *s, int before) {
    if ((s[-1] & 0xC0u) != 0x80u) return 1;
    for (int k = 2; k <= 4 && k <= before; ++k)
        if (split_unit_len(s - k, k) == k) return k;
    return 1;
}

// The class of the unit of `len` bytes at q.
SPLIT_FN uint32_t split_class(const SplitTable &t, const uint8_t *q, int len) {
    const uint32_t b0 = q[0];
    if (len == 1) {
        if ((b0 | 0x20u) - 'a' < 26u) return kSplitL;
        if (b0 - '0' < 10u) return kSplitN;
        if (b0 == 0x20u || b0 - 0x09u < 5u) return kSplitS;
        return kSplitO;
    }
    uint32_t cp;
    if (len == 2) cp = (b0 & 0x1Fu) << 6 | (q[1] & 0x3Fu);
    else if (len == 3) cp = (b0 & 0x0Fu) << 12 | (q[1] & 0x3Fu) << 6 | (q[2] & 0x3Fu);
    else cp = (b0 & 0x07u) << 18 | (q[1] & 0x3Fu) << 12 | (q[2] & 0x3Fu) << 6 | (q[3] & 0x3Fu);
    const uint32_t blk = t.stage1[cp >> 8];   // (a well-formed sequence is at most U+10FFFF: inside the first stage)
    return (t.stage2[blk * kSplitBlockBytes + ((cp & 255u) >> 2)] >> (2u * (cp & 3u))) & 3u;
}

// K of the ' at w - back (back in 1 .. 3): `before` bytes in front of w and `ahead` from w on belong to the document.
SPLIT_FN int split_contraction(const SplitTable &t, const uint8_t *w, int back, int before, int ahead) {
    if (back > before) return 0;
    const uint8_t *q = w - back;
    if (q[0] != '\'') return 0;
    const int avail = ahead + back;
    int k = 0;
    if (avail >= 2 && (q[1] == 's' || q[1] == 't' || q[1] == 'm' || q[1] == 'd')) k = 2;
    else if (avail >= 3 && ((q[1] == 'r' && q[2] == 'e') || (q[1] == 'v' && q[2] == 'e') || (q[1] == 'l' && q[2] == 'l'))) k = 3;
    if (!k || back == before) return k;   // (the document's first unit: AS holds)
    const int pl = split_prev_len(q, before - back);
    const uint32_t pc = split_class(t, q - pl, pl);
    if (pc == kSplitL || pc == kSplitN) return k;
    return pc == kSplitS && q[-1] != 0x20u ? k : 0;   // (a unit whose last byte is 0x20 is the space)
}

// Whether a word starts at the byte w.  Of w's document the bytes w[-before .. ahead - 1] may be read: before = min(bytes in front of
// w, kSplitBack), ahead = min(bytes from w to the document's end, kSplitAhead) >= 1.
SPLIT_FN bool split_start(const SplitTable &t, const uint8_t *w, int before, int ahead, int rule) {
    if ((w[0] & 0xC0u) == 0x80u)   // inside a well-formed sequence: no unit starts here
        for (int k = 1; k <= 3 && k <= before; ++k)
            if (split_unit_len(w - k, ahead + k) > k) return false;
    if (before == 0) return true;
    const int len0 = split_unit_len(w, ahead);
    const uint32_t c0 = split_class(t, w, len0);
    const int len1 = split_prev_len(w, before);
    const uint32_t c1 = split_class(t, w - len1, len1);
    const bool s0 = c0 == kSplitS, s1 = c1 == kSplitS;
    if (rule == DAAC_SPLIT_WHITESPACE) return s0 != s1;
    if (s0 && s1) {
        if (len0 >= ahead) return false;
        const int len2 = split_unit_len(w + len0, ahead - len0);
        return split_class(t, w + len0, len2) != kSplitS;
    }
    if (s0) return true;
    if (s1) return w[-1] != 0x20u;
    const int k2 = split_contraction(t, w, 2, before, ahead);
    if (c0 == kSplitL && (k2 == 3 || split_contraction(t, w, 1, before, ahead) != 0)) return false;
    if (k2 == 2 || split_contraction(t, w, 3, before, ahead) == 3) return true;
    return c0 != c1;
}

// before and ahead of a position from the mark bits around it: bit k of `win` is the mark of position p - kSplitBack + k,
// k < kSplitBack + kSplitAhead.  A mark at or in front of p ends the look-back, a mark behind p the look-ahead.
SPLIT_FN void split_reach(uint32_t win, int &before, int &ahead) {
    const uint32_t back = win & ((2u << kSplitBack) - 2u);   // positions p - kSplitBack + 1 .. p
    before = back ? kSplitBack - (31 - __builtin_clz(back)) : kSplitBack;
    const uint32_t fwd = (win >> (kSplitBack + 1)) & ((1u << (kSplitAhead - 1)) - 1u);   // positions p + 1 .. p + kSplitAhead - 1
    ahead = fwd ? __builtin_ctz(fwd) + 1 : kSplitAhead;
}

#ifndef DAAC_SPLIT_HOST
// ------------------------------------------------------------------------------------------------------- kernels and launchers
constexpr uint32_t kSplitTileWords = kSplitTile / 64;     // mask words of a tile
constexpr uint32_t kSplitMarkWords = kSplitTile / 32;     // mark words of a tile
constexpr uint32_t kSplitMaxBlocks = 1u << 20;            // workgroups of a pass; they stride over the tiles
static_assert(kSplitTile % kSplitLanes == 0 && kSplitLanes % 64 == 0, "a wave's positions are one mask word");
static_assert(kSplitBack + kSplitAhead <= 32 && kSplitBack < 32, "the mark window is one 32-bit word");

__global__ __launch_bounds__(256) void split_mark_kernel(const SplitArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride) {
        const uint64_t off = a.doc_off[d];
        if (off < a.base || off - a.base > a.total) continue;   // (never: the driver has checked the offsets)
        const uint64_t p = off - a.base;
        if (d < a.n_docs && a.doc_off[d + 1] <= off) continue;  // an empty document
        atomicOr(&a.marks[p >> 5], 1u << (p & 31u));
    }
}

__global__ __launch_bounds__(kSplitLanes) void split_flag_kernel(const SplitArgs a) {
    __shared__ uint8_t s_txt[kSplitTile + 32];             // entry kSplitBack + l: the byte of the tile's position l
    __shared__ uint32_t s_mark[kSplitMarkWords + 2];       // entry 1 + j: the tile's mark word j
    __shared__ uint32_t s_cnt[kSplitLanes / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_mark = a.tiles * kSplitMarkWords + 1;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint64_t base = tile * kSplitTile;
        for (uint32_t i = tid; i < kSplitTile + kSplitBack + kSplitAhead - 1; i += kSplitLanes) {
            const uint64_t p = base + i;   // the position + kSplitBack
            s_txt[i] = p >= static_cast<uint64_t>(kSplitBack) && p - kSplitBack < a.total ? a.text[p - kSplitBack] : static_cast<uint8_t>(0);
        }
        for (uint32_t i = tid; i < kSplitMarkWords + 2; i += kSplitLanes) {
            const uint64_t w = tile * kSplitMarkWords + i;   // the word + 1
            s_mark[i] = w >= 1 && w - 1 < n_mark ? a.marks[w - 1] : 0u;
        }
        __syncthreads();
        uint32_t cnt = 0;
        for (uint32_t it = 0; it < kSplitTile / kSplitLanes; ++it) {
            const uint32_t l = it * kSplitLanes + tid;
            const uint64_t p = base + l;
            bool f = false;
            if (p < a.total) {
                const uint32_t q = l + 32u - kSplitBack;   // the bit of position p - kSplitBack in s_mark
                const uint64_t two = static_cast<uint64_t>(s_mark[(q >> 5) + 1]) << 32 | s_mark[q >> 5];
                int before, ahead;
                split_reach(static_cast<uint32_t>(two >> (q & 31u)), before, ahead);
                f = split_start(a.tab, &s_txt[l + kSplitBack], before, ahead, a.rule);
            }
            const unsigned long long m = __ballot(f);
            if ((tid & 63u) == 0) {
                a.masks[p >> 6] = m;
                cnt += static_cast<uint32_t>(__popcll(m));
            }
        }
        if ((tid & 63u) == 0) s_cnt[tid >> 6] = cnt;
        __syncthreads();
        if (tid == 0) {
            unsigned long long sum = 0;
            for (uint32_t i = 0; i < kSplitLanes / 64; ++i) sum += s_cnt[i];
            a.counts[tile] = sum;
        }
        __syncthreads();   // the next tile is staged over this one
    }
}

__global__ __launch_bounds__(kSplitLanes) void split_scatter_kernel(const SplitArgs a) {
    __shared__ uint32_t s_pre[kSplitTileWords];   // the set bits of the tile's mask words in front of word j
    const uint32_t tid = threadIdx.x;
    const unsigned long long n_words = *a.n_words;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        if (tid == 0) {
            uint32_t run = 0;
            for (uint32_t j = 0; j < kSplitTileWords; ++j) {
                s_pre[j] = run;
                run += static_cast<uint32_t>(__popcll(a.masks[tile * kSplitTileWords + j]));
            }
        }
        __syncthreads();
        const unsigned long long first = a.counts[tile];
        for (uint32_t it = 0; it < kSplitTile / kSplitLanes; ++it) {
            const uint32_t l = it * kSplitLanes + tid;
            const unsigned long long m = a.masks[tile * kSplitTileWords + (l >> 6)];
            const uint32_t bit = l & 63u;
            if ((m >> bit) & 1ull) {
                const unsigned long long rank = first + s_pre[l >> 6] + static_cast<uint32_t>(__popcll(m & ((1ull << bit) - 1ull)));
                if (rank < n_words) a.word_offsets[rank] = a.base + tile * kSplitTile + l;
            }
        }
        __syncthreads();
    }
}

// doc_words[d] = the word starts in front of document d's first position; the lane behind the last document closes both lists
__global__ __launch_bounds__(256) void split_docs_kernel(const SplitArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const unsigned long long n_words = *a.n_words;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride) {
        const uint64_t off = a.doc_off[d];
        const uint64_t p = off < a.base ? 0 : off - a.base;
        unsigned long long rank = n_words;
        if (p < a.total) {
            const uint64_t tile = p / kSplitTile;
            const uint32_t l = static_cast<uint32_t>(p % kSplitTile);
            rank = a.counts[tile];
            for (uint32_t j = 0; j < (l >> 6); ++j) rank += static_cast<uint32_t>(__popcll(a.masks[tile * kSplitTileWords + j]));
            rank += static_cast<uint32_t>(__popcll(a.masks[tile * kSplitTileWords + (l >> 6)] & ((1ull << (l & 63u)) - 1ull)));
        }
        a.doc_words[d] = rank;
        if (d == a.n_docs) a.word_offsets[n_words] = a.base + a.total;
    }
}

__global__ __launch_bounds__(256) void offsets_compose_kernel(const unsigned long long *inner, const unsigned long long *outer, uint64_t n, unsigned long long *out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = inner[outer[i]];
}

__global__ __launch_bounds__(256) void spans_rebase_kernel(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *word_offsets,
                                                           const unsigned long long *doc_words, const unsigned long long *doc_off, uint64_t n_words, uint64_t n_docs) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < n_words; w += stride) {
        uint64_t lo = 0, hi = n_docs;   // the last document d with doc_words[d] <= w: the word's (empty documents share an entry)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (doc_words[mid] <= w) lo = mid; else hi = mid;
        }
        const unsigned long long delta = word_offsets[w] - doc_off[lo];
        const unsigned long long e = tok_offsets[w + 1];
        for (unsigned long long t = tok_offsets[w]; t < e; ++t) {
            spans[2 * t] += delta;
            spans[2 * t + 1] += delta;
        }
    }
}

static uint32_t split_grid(uint64_t items, uint32_t per_block, uint32_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_split_marks(const SplitArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(split_mark_kernel, dim3(split_grid(a.n_docs + 1, 256, 4096)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_split_flags(const SplitArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(split_flag_kernel, dim3(split_grid(a.tiles, 1, kSplitMaxBlocks)), dim3(kSplitLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_split_scatter(const SplitArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(split_scatter_kernel, dim3(split_grid(a.tiles, 1, kSplitMaxBlocks)), dim3(kSplitLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(split_docs_kernel, dim3(split_grid(a.n_docs + 1, 256, 4096)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_offsets_compose(const unsigned long long *inner, const unsigned long long *outer, uint64_t n, unsigned long long *out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(offsets_compose_kernel, dim3(split_grid(n, 256, 4096)), dim3(256), 0, stream, inner, outer, n, out);
    return hipGetLastError();
}

hipError_t launch_spans_rebase(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *word_offsets,
                               const unsigned long long *doc_words, const unsigned long long *doc_off, uint64_t n_words, uint64_t n_docs, hipStream_t stream) {
    if (n_words == 0 || n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(spans_rebase_kernel, dim3(split_grid(n_words, 256, 4096)), dim3(256), 0, stream, spans, tok_offsets, word_offsets, doc_words, doc_off,
                       n_words, n_docs);
    return hipGetLastError();
}
#endif

}  // namespace daac
