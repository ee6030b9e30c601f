// normalize_batch for gfx950 (daac_normalize_batch, daac_normalize, daac_spans_to_source): a per-code-point rewrite of a batch of
// documents as two streaming passes with one lane per byte around an exclusive sum.  normalize.hpp has the scratch layout,
// include/daachorse_amd.h the definition.
//
//   marks    split_kernels.hip's: one lane per document sets the bit of a non-empty document's first position, and bit `total`.
//   count    a workgroup takes a tile of kNormTile positions.  It stages the tile's bytes with kNormBack bytes in front and
//            kNormAhead - 1 behind, and the tile's mark bits with a word on either side, in LDS.  A lane takes kNormPerLane consecutive
//            positions: the mark bits around a position say how many of the staged bytes belong to its document (norm_reach),
//            norm_unit says whether a unit starts there, which, and how many bytes its image has.  The tile's sum goes to counts[tile].
//   write    behind the exclusive sum of the counts: the same staging and the same decisions, an exclusive sum of the image lengths over
//            the tile's lanes (wave shuffles, the waves' totals in LDS), and the lane that owns a unit stores its image at
//            counts[tile] + that sum, byte by byte, with the unit's offset in its document for every byte where `src` is asked for.  A
//            unit that straddles a tile edge is owned by the tile of its first byte.  A lane whose position carries a mark looks up its
//            document by bisection and stores its rank: out_offsets of a non-empty document.
//   docs     one lane per document: the entry of an empty document (that of the document behind it, or out_len) and the closing entry.
// Both passes run one workgroup per tile.  The write pass keeps what a lane found at its positions (entry, unit and image length) in LDS
// for the lane itself, so that its store loop is rolled: nothing of the four units is held in registers at once.
//
// A document's first position for `src`: the last mark at or in front of the position inside the tile, else the document that holds the
// tile's first position, found once per tile by bisection.
//
// Reads stay inside [offsets[0], offsets[n]): a staged byte outside it is 0 and no decision reads it, because position 0 and position
// `total` carry marks.  Writes: counts by the lane that owns them, out and src guarded by out_len, out_offsets by the document's number.
// Plain vector stores, no atomics, no inline assembly.
//
// The per-position functions below are plain C++: with DAAC_NORMALIZE_HOST defined this file compiles without HIP and a host program
// evaluates them at every position of documents held in buffers of exactly their size (tests/native/normalize_check.cpp, under ASan and
// UBSan).
#ifndef DAAC_NORMALIZE_HOST
#include <hip/hip_runtime.h>
#define NORM_FN static __device__ __forceinline__
#else
#define NORM_FN static inline
#endif

#include <cstdint>

#include "normalize.hpp"

namespace daac {

// The bytes of the unit that begins at q, of whose document `avail` >= 1 bytes from q on may be read: 2 .. 4 for a well-formed
// sequence (Unicode Table 3-7) that fits, else 1.  The splitter's rule (split_unit_len), byte for byte.
NORM_FN int norm_unit_len(const uint8_t *q, int avail) {
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

// before and ahead of a position from the mark bits around it: bit k of `win` is the mark of position p - kNormBack + k,
// k < kNormBack + kNormAhead.  A mark at or in front of p ends the look-back, a mark behind p the look-ahead.
NORM_FN void norm_reach(uint32_t win, int &before, int &ahead) {
    const uint32_t back = win & ((2u << kNormBack) - 2u);   // positions p - kNormBack + 1 .. p
    before = back ? kNormBack - (31 - __builtin_clz(back)) : kNormBack;
    const uint32_t fwd = (win >> (kNormBack + 1)) & ((1u << (kNormAhead - 1)) - 1u);   // positions p + 1 .. p + kNormAhead - 1
    ahead = fwd ? __builtin_ctz(fwd) + 1 : kNormAhead;
}

// The window of norm_reach for the position whose mark is bit q + kNormBack of the words at `m`.
NORM_FN uint32_t norm_window(const uint32_t *m, uint32_t q) {
    const uint64_t two = static_cast<uint64_t>(m[(q >> 5) + 1]) << 32 | m[q >> 5];
    return static_cast<uint32_t>(two >> (q & 31u));
}

// The code point of the well-formed sequence of len >= 2 bytes at q.
NORM_FN uint32_t norm_cp(const uint8_t *q, int len) {
    const uint32_t b0 = q[0];
    if (len == 2) return (b0 & 0x1Fu) << 6 | (q[1] & 0x3Fu);
    if (len == 3) return (b0 & 0x0Fu) << 12 | (q[1] & 0x3Fu) << 6 | (q[2] & 0x3Fu);
    return (b0 & 0x07u) << 18 | (q[1] & 0x3Fu) << 12 | (q[2] & 0x3Fu) << 6 | (q[3] & 0x3Fu);
}

struct NormUnit {
    uint32_t len;     // the unit's bytes; 0: no unit starts here
    uint32_t entry;   // its table entry (0: copied)
    uint32_t cp;      // its code point (an ill-formed byte: the byte)
    uint32_t image;   // the bytes of its image
};

// The unit that starts at the byte w, if one does.  Of w's document the bytes w[-before .. ahead - 1] may be read: before = min(bytes in
// front of w, kNormBack), ahead = min(bytes from w to the document's end, kNormAhead) >= 1.
NORM_FN NormUnit norm_unit(const NormTable &t, const uint8_t *w, int before, int ahead) {
    NormUnit u{0, 0, 0, 0};
    const uint32_t b0 = w[0];
    if (b0 < 0x80u) {   // the direct path
        u.len = 1;
        u.cp = b0;
        u.entry = t.ascii[b0];
    } else {
        if ((b0 & 0xC0u) == 0x80u)   // inside a well-formed sequence: no unit starts here
            for (int k = 1; k <= 3 && k <= before; ++k)
                if (norm_unit_len(w - k, ahead + k) > k) return u;
        const int len = norm_unit_len(w, ahead);
        u.len = static_cast<uint32_t>(len);
        if (len == 1) { u.cp = b0; u.image = 1; return u; }   // an ill-formed byte is copied
        u.cp = norm_cp(w, len);
        // (a well-formed sequence is at most U+10FFFF: inside the first stage)
        u.entry = t.stage2[static_cast<uint32_t>(t.stage1[u.cp >> 8]) * kNormBlock + (u.cp & 255u)];
    }
    const uint32_t kind = u.entry & 7u;
    if (kind == kNormCopy) u.image = u.len;
    else if (kind == kNormReplace) u.image = (u.entry >> 3) & 255u;
    else if (kind == kNormPad) u.image = u.len + 2u;
    else if (kind == kNormHangul) u.image = (u.cp - kHangulFirst) % 28u ? 9u : 6u;   // two or three jamo of three bytes
    return u;   // (kNormDelete: 0)
}

NORM_FN void norm_put3(uint8_t *out, uint32_t cp) {   // U+0800 .. U+FFFF
    out[0] = static_cast<uint8_t>(0xE0u | cp >> 12);
    out[1] = static_cast<uint8_t>(0x80u | ((cp >> 6) & 0x3Fu));
    out[2] = static_cast<uint8_t>(0x80u | (cp & 0x3Fu));
}

// Stores the u.image bytes of the image of the unit u at w.
NORM_FN void norm_store(const NormTable &t, const NormUnit &u, const uint8_t *w, uint8_t *out) {
    const uint32_t kind = u.entry & 7u;
    if (kind == kNormCopy || kind == kNormPad) {
        if (kind == kNormPad) { *out++ = 0x20u; out[u.len] = 0x20u; }
        for (uint32_t k = 0; k < u.len; ++k) out[k] = w[k];
    } else if (kind == kNormReplace) {
        const uint8_t *from = t.pool + (u.entry >> 11);
        for (uint32_t k = 0; k < u.image; ++k) out[k] = from[k];
    } else if (kind == kNormHangul) {   // Unicode 3.12: L V or L V T
        const uint32_t s = u.cp - kHangulFirst;
        norm_put3(out, 0x1100u + s / 588u);
        norm_put3(out + 3, 0x1161u + s % 588u / 28u);
        if (s % 28u) norm_put3(out + 6, 0x11A7u + s % 28u);
    }
}

// The first index i in [0, n) with v[i] > x, n if there is none: v does not decrease.
NORM_FN uint64_t norm_upper_bound(const unsigned long long *v, uint64_t n, unsigned long long x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Token t's span, relative to its normalized document, made relative to the input document.  start -> src[start]; end -> src[end - 1]
// plus the bytes of the input unit there; an empty span at p -> src[p] twice, src at the document's output length being its input length.
NORM_FN void norm_span_to_source(unsigned long long *span, uint64_t t, const unsigned long long *tok_offsets, const unsigned long long *out_offsets, const uint32_t *src,
                                 const uint8_t *hay, const unsigned long long *doc_off, uint64_t n_docs) {
    const uint64_t d = norm_upper_bound(tok_offsets, n_docs + 1, t) - 1;   // the last document with tok_offsets[d] <= t: it has the token
    if (d >= n_docs) return;   // (never: t < tok_offsets[n_docs])
    const unsigned long long ob = out_offsets[d], ol = out_offsets[d + 1] - ob, ib = doc_off[d], il = doc_off[d + 1] - ib;
    const unsigned long long s = span[0], e = span[1];
    if (s > e || e > ol) return;   // (never: a span lies inside its document)
    if (s == e) {
        span[0] = span[1] = s < ol ? src[ob + s] : il;
        return;
    }
    const unsigned long long last = src[ob + e - 1];
    span[0] = src[ob + s];
    span[1] = last + (last < il ? static_cast<unsigned>(norm_unit_len(hay + ib + last, il - last < 4 ? static_cast<int>(il - last) : 4)) : 0u);
}

#ifndef DAAC_NORMALIZE_HOST
// ------------------------------------------------------------------------------------------------------- kernels and launchers
constexpr uint32_t kNormMarkWords = kNormTile / 32;     // mark words of a tile
constexpr uint32_t kNormWaves = kNormLanes / 64;
constexpr uint32_t kNormMaxBlocks = 1u << 20;           // the grid's first dimension; its second counts on behind that many tiles
static_assert(kNormBack + kNormAhead <= 32, "the mark window is one 32-bit word");
static_assert(kNormBack + kNormAhead - 1 <= 16, "the staged text has 16 bytes beyond the tile");

struct NormTileLds {
    uint8_t txt[kNormTile + 16];             // entry kNormBack + l: the byte of the tile's position l
    uint32_t mark[kNormMarkWords + 2];       // entry 1 + j: the tile's mark word j
    int32_t last[kNormMarkWords];            // the last marked position of the tile in front of mark word j, -1: none
    unsigned long long doc0;                 // the first position of the document that holds the tile's first position
    uint32_t wave[kNormWaves];               // the waves' sums
};
struct NormKeepLds {                         // the write pass: what a lane found at its positions, for itself
    uint32_t entry[kNormTile];               // entry j * kNormLanes + lane: the table entry of the unit at the lane's position j
    uint16_t shape[kNormTile];               // ... its bytes | its image's bytes << 4
};

// A workgroup takes one tile: with no loop over tiles nothing of a tile's work is kept in registers for the next one.
static __device__ __forceinline__ uint64_t norm_tile_of_block() { return static_cast<uint64_t>(blockIdx.y) * gridDim.x + blockIdx.x; }

// Stages a tile.  Ends behind a barrier.
static __device__ __forceinline__ void norm_stage(const NormArgs &a, uint64_t tile, NormTileLds &s) {
    const uint32_t tid = threadIdx.x;
    const uint64_t n_mark = a.tiles * kNormMarkWords + 1;
    const uint64_t base = tile * kNormTile;
    for (uint32_t i = tid; i < kNormTile + kNormBack + kNormAhead - 1; i += kNormLanes) {
        const uint64_t p = base + i;   // the position + kNormBack
        s.txt[i] = p >= static_cast<uint64_t>(kNormBack) && p - kNormBack < a.total ? a.text[p - kNormBack] : static_cast<uint8_t>(0);
    }
    for (uint32_t i = tid; i < kNormMarkWords + 2; i += kNormLanes) {
        const uint64_t w = tile * kNormMarkWords + i;   // the word + 1
        s.mark[i] = w >= 1 && w - 1 < n_mark ? a.marks[w - 1] : 0u;
    }
    __syncthreads();
}

// The units of the lane's kNormPerLane positions; -> the bytes of their images.  keep: NULL, or where the units are kept.
static __device__ __forceinline__ uint32_t norm_lane_units(const NormArgs &a, uint64_t base, const NormTileLds &s, NormKeepLds *keep) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kNormPerLane; ++j) {
        const uint32_t l = threadIdx.x * kNormPerLane + j;
        NormUnit u{0, 0, 0, 0};
        if (base + l < a.total) {
            int before, ahead;
            norm_reach(norm_window(s.mark, l + 32u - kNormBack), before, ahead);
            u = norm_unit(a.tab, &s.txt[l + kNormBack], before, ahead);
        }
        if (keep) {
            keep->entry[j * kNormLanes + threadIdx.x] = u.entry;
            keep->shape[j * kNormLanes + threadIdx.x] = static_cast<uint16_t>(u.len | u.image << 4);   // (at most 4 and kNormMaxLen)
        }
        sum += u.image;
    }
    return sum;
}

__global__ __launch_bounds__(kNormLanes) void normalize_count_kernel(const NormArgs a) {
    __shared__ NormTileLds s;
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = norm_tile_of_block();
    if (tile >= a.tiles) return;
    norm_stage(a, tile, s);
    uint32_t sum = norm_lane_units(a, tile * kNormTile, s, nullptr);
    for (int o = 32; o; o >>= 1) sum += __shfl_down(sum, o);
    if ((tid & 63u) == 0) s.wave[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long all = 0;
        for (uint32_t i = 0; i < kNormWaves; ++i) all += s.wave[i];
        a.counts[tile] = all;
    }
}

template <bool kSrc>
__global__ __launch_bounds__(kNormLanes) void normalize_write_kernel(const NormArgs a) {
    __shared__ NormTileLds s;
    __shared__ NormKeepLds keep;
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = norm_tile_of_block();
    if (tile >= a.tiles) return;
    const unsigned long long out_len = *a.out_len;
    const uint64_t base = tile * kNormTile;
    norm_stage(a, tile, s);
    const uint32_t own = norm_lane_units(a, base, s, &keep);
    uint32_t incl = own;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o);
        if ((tid & 63u) >= static_cast<uint32_t>(o)) incl += up;
    }
    if ((tid & 63u) == 63u) s.wave[tid >> 6] = incl;
    if (kSrc && tid == 0) {
        int32_t run = -1;
        for (uint32_t j = 0; j < kNormMarkWords; ++j) {
            s.last[j] = run;
            const uint32_t m = s.mark[1 + j];
            if (m) run = static_cast<int32_t>(j * 32u + 31u - static_cast<uint32_t>(__builtin_clz(m)));
        }
        // the last offset that is not behind the tile's first position (offsets[0] is none)
        s.doc0 = a.doc_off[norm_upper_bound(a.doc_off, a.n_docs + 1, a.base + base) - 1] - a.base;
    }
    __syncthreads();
    unsigned long long pos = a.counts[tile] + (incl - own);
    for (uint32_t w = 0; w < (tid >> 6); ++w) pos += s.wave[w];
#pragma unroll 1
    for (uint32_t j = 0; j < kNormPerLane; ++j) {
        const uint32_t l = tid * kNormPerLane + j;
        const uint64_t p = base + l;
        const uint32_t m = s.mark[1 + (l >> 5)];
        const uint32_t shape = keep.shape[j * kNormLanes + tid];
        NormUnit u{shape & 15u, keep.entry[j * kNormLanes + tid], 0, shape >> 4};
        if ((u.entry & 7u) == kNormHangul) u.cp = norm_cp(&s.txt[l + kNormBack], 3);
        if (p < a.total && ((m >> (l & 31u)) & 1u)) {   // a non-empty document starts here: the last one with this offset
            const uint64_t d = norm_upper_bound(a.doc_off, a.n_docs + 1, a.base + p) - 1;
            if (d < a.n_docs) a.out_offsets[d] = pos;
        }
        if (u.image && pos + u.image <= out_len) {
            norm_store(a.tab, u, &s.txt[l + kNormBack], a.out + pos);
            if (kSrc) {
                const uint32_t at = m & (0xFFFFFFFFu >> (31u - (l & 31u)));   // the marks of the word up to and including l
                const unsigned long long first = at ? base + (l & ~31u) + 31u - static_cast<uint32_t>(__builtin_clz(at))
                                                     : s.last[l >> 5] >= 0 ? base + static_cast<uint32_t>(s.last[l >> 5]) : s.doc0;
                const uint32_t off = static_cast<uint32_t>(p - first);
                for (uint32_t k = 0; k < u.image; ++k) a.src[pos + k] = off;
            }
        }
        pos += u.image;
    }
}

// The entries the write pass has not stored: an empty document's (the rank of the document behind it) and the closing one.
__global__ __launch_bounds__(256) void normalize_docs_kernel(const NormArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const unsigned long long out_len = *a.out_len;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride) {
        const unsigned long long off = a.doc_off[d];
        if (off >= a.base + a.total) { a.out_offsets[d] = out_len; continue; }
        if (d < a.n_docs && a.doc_off[d + 1] > off) continue;   // not empty: the write pass has stored it
        const uint64_t e = norm_upper_bound(a.doc_off, a.n_docs + 1, off) - 1;   // the non-empty document at this offset (e > d)
        a.out_offsets[d] = a.out_offsets[e];
    }
}

__global__ __launch_bounds__(256) void normalize_longest_kernel(const unsigned long long *doc_off, uint64_t n_docs, unsigned long long *longest) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned long long best = 0;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d < n_docs; d += stride) {
        const unsigned long long len = doc_off[d + 1] - doc_off[d];
        best = len > best ? len : best;
    }
    if (best) atomicMax(longest, best);
}

__global__ __launch_bounds__(256) void spans_to_source_kernel(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *out_offsets,
                                                              const uint32_t *src, const uint8_t *hay, const unsigned long long *doc_off, uint64_t n_docs,
                                                              uint64_t n_tokens) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_tokens; t += stride)
        norm_span_to_source(spans + 2 * t, t, tok_offsets, out_offsets, src, hay, doc_off, n_docs);
}

static uint32_t norm_grid(uint64_t items, uint32_t per_block, uint32_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

// a workgroup per tile
static bool norm_tile_grid(uint64_t tiles, dim3 &grid) {
    const uint32_t gx = norm_grid(tiles, 1, kNormMaxBlocks), gy = static_cast<uint32_t>((tiles + gx - 1) / gx);
    grid = dim3(gx, gy);
    return gy <= 65535u;   // (2^36 tiles: never)
}

hipError_t launch_normalize_count(const NormArgs &a, hipStream_t stream) {
    dim3 grid;
    if (!norm_tile_grid(a.tiles, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(normalize_count_kernel, grid, dim3(kNormLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_normalize_write(const NormArgs &a, hipStream_t stream) {
    dim3 grid;
    if (!norm_tile_grid(a.tiles, grid)) return hipErrorInvalidValue;
    if (a.src) hipLaunchKernelGGL(normalize_write_kernel<true>, grid, dim3(kNormLanes), 0, stream, a);
    else hipLaunchKernelGGL(normalize_write_kernel<false>, grid, dim3(kNormLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(normalize_docs_kernel, dim3(norm_grid(a.n_docs + 1, 256, 4096)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_normalize_longest(const unsigned long long *doc_off, uint64_t n_docs, unsigned long long *longest, hipStream_t stream) {
    if (n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(normalize_longest_kernel, dim3(norm_grid(n_docs, 256, 4096)), dim3(256), 0, stream, doc_off, n_docs, longest);
    return hipGetLastError();
}

hipError_t launch_spans_to_source(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *out_offsets, const uint32_t *src,
                                  const uint8_t *hay, const unsigned long long *doc_off, uint64_t n_docs, uint64_t n_tokens, hipStream_t stream) {
    if (n_tokens == 0 || n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(spans_to_source_kernel, dim3(norm_grid(n_tokens, 256, 4096)), dim3(256), 0, stream, spans, tok_offsets, out_offsets, src, hay, doc_off,
                       n_docs, n_tokens);
    return hipGetLastError();
}
#endif

}  // namespace daac
