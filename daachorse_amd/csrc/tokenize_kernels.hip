// tokenize for gfx950 (daac_tokenize, daac_tokenize_batch): the passes between the tuple list and the token list.  tokenize.hpp has the
// definitions (absolute positions, A_i, D_d, flagged bytes, rank, E_i) and the two index formulas everything below rests on.
//
//   prep    one lane per match: A_i (a batch: the match's document by a binary search in the CSR offsets) and "the match is empty".
//   tiles   one lane per tile of kTokTile bytes: how many matches end before the tile's first byte, how many documents begin before it.
//   count   input-parallel: a workgroup owns a tile, a lane 16 bytes of it.  The lane walks the matches and documents that touch its
//           bytes, builds the 16-bit mask of flagged bytes and the workgroup sums the popcounts.
//   write   the same masks again; wave and workgroup prefix sums of the popcounts on top of the tile's base give rank(p), and the lane
//           walks its events in position order: a gap token's end (written by whoever follows it), tok_offsets of the documents that
//           begin here, the empty matches here, the byte token here.
//
// Every output word is written by exactly one lane, at an index that is a sum of counts: no atomics, integer work only, so the result is
// a function of the input alone.  The text is read inside [hay, hay + len) only: 16 bytes at once where all 16 are in range.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "tokenize.hpp"
#include "../../include/daachorse_amd.h"

namespace daac {

static __device__ __forceinline__ uint64_t tok_seg_end(const uint4 &t) { return static_cast<uint64_t>(t.x) | (static_cast<uint64_t>(t.y) << 32); }
static __device__ __forceinline__ uint64_t doc_begin(const TokenizeArgs &a, uint64_t d) { return a.doc_off[d] - a.doc_off[0]; }

__global__ __launch_bounds__(256) void tokenize_prep_kernel(const TokenizeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= a.k; i += stride) {
        if (i == a.k) { a.epre[i] = 0; continue; }   // (the sum's entry k is the total)
        const uint4 t = a.seg[i];
        uint64_t end = tok_seg_end(t);
        if (a.doc_first) {
            uint64_t lo = 0, hi = a.n_docs;  // the match's document: the last d with doc_first[d] <= i (doc_first[n_docs] = k > i, so it has matches)
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (a.doc_first[mid] <= i) lo = mid; else hi = mid;
            }
            end += doc_begin(a, lo);
        }
        a.aend[i] = end;
        a.epre[i] = t.z == 0;
    }
}

__global__ __launch_bounds__(256) void tokenize_tiles_kernel(const TokenizeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t <= a.tiles; t += stride) {
        const uint64_t q = t * kTokTile;   // (entry `tiles`: q > len, so every match and every document, D_n = len included)
        uint64_t lo = 0, hi = a.k;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (a.aend[mid] < q) lo = mid + 1; else hi = mid;
        }
        a.tile_lo[t] = lo;
        lo = 0; hi = a.n_docs + 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (doc_begin(a, mid) < q) lo = mid + 1; else hi = mid;
        }
        a.tile_doc[t] = lo;
        if (t == a.tiles) a.tile_cnt[t] = 0;
    }
}

// What a lane knows of its positions q0 .. q0 + 15 (bit b: position q0 + b) before any prefix sum.
struct TokLane {
    uint64_t q0;
    uint64_t j0;        // matches with A_i < q0: the walk over the lane's matches begins here
    uint64_t d0;        // documents with D_d < q0
    uint32_t flag;      // a byte token begins at this byte
    uint32_t cov;       // the byte lies in a non-empty match
    uint32_t mst;       // a non-empty match begins at this byte
    uint32_t ends;      // a match ends or a document begins at this position (position len included)
    uint32_t w0, w1, w2, w3;   // the lane's bytes, where the gap rule looks at them
    bool prev_cov;      // byte q0 - 1 lies in a non-empty match
    bool live;          // q0 <= len
};

static __device__ __forceinline__ uint32_t lane_word(const TokLane &s, uint32_t x) {
    const uint32_t w0 = s.w0, w1 = s.w1, w2 = s.w2, w3 = s.w3;   // (values, not a choice between addresses: the lane stays in registers)
    return x < 2 ? (x == 0 ? w0 : w1) : (x == 2 ? w2 : w3);
}
static __device__ __forceinline__ uint32_t bits_below(uint32_t b) { return (1u << b) - 1u; }   // b <= 16

// `text`: the pass needs the lane's bytes (DAAC_GAP_CHARS always does)
static __device__ __forceinline__ TokLane tok_lane(const TokenizeArgs &a, uint64_t t, bool text) {
    TokLane s{};
    s.q0 = t * kTokTile + static_cast<uint64_t>(threadIdx.x) * 16;
    s.live = s.q0 <= a.len;
    if (!s.live) return s;
    const uint64_t q0 = s.q0;
    const uint32_t nvalid = static_cast<uint32_t>(std::min<uint64_t>(16, a.len - q0));
    // the matches: A_i >= q0 from j0 on, and starts do not decrease, so the walk ends at the first match that begins beyond the lane
    uint64_t lo = a.tile_lo[t], hi = a.tile_lo[t + 1];
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a.aend[mid] < q0) lo = mid + 1; else hi = mid;
    }
    s.j0 = lo;
    for (uint64_t i = lo; i < a.k; ++i) {
        const uint64_t e = a.aend[i];
        const uint32_t l = a.seg[i].z;
        const uint64_t st = e - l;
        if (st >= q0 + 16) break;
        if (e - q0 < 16) s.ends |= 1u << static_cast<uint32_t>(e - q0);
        if (l) {
            const uint32_t from = st > q0 ? static_cast<uint32_t>(st - q0) : 0u;
            const uint32_t to = e - q0 < 16 ? static_cast<uint32_t>(e - q0) : 16u;
            s.cov |= bits_below(to) & ~bits_below(from);
            if (st >= q0) s.mst |= 1u << from; else s.prev_cov = true;
        }
    }
    // the documents that begin at the lane's positions (D_n = len among them)
    lo = a.tile_doc[t]; hi = a.tile_doc[t + 1];
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (doc_begin(a, mid) < q0) lo = mid + 1; else hi = mid;
    }
    s.d0 = lo;
    for (uint64_t d = lo; d <= a.n_docs; ++d) {
        const uint64_t at = doc_begin(a, d);
        if (at - q0 >= 16) break;
        s.ends |= 1u << static_cast<uint32_t>(at - q0);
    }
    uint32_t rule = 0;
    if (a.gap == DAAC_GAP_UNK) rule = s.ends;
    else if (a.gap == DAAC_GAP_BYTES) rule = 0xffffu;
    if (text) {
        uint32_t w[4] = {0, 0, 0, 0};   // (indexed by constants only)
        if (nvalid == 16) {
            uint4 v;
            __builtin_memcpy(&v, a.hay + q0, 16);   // (any alignment)
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {   // the text's last granule
#pragma unroll
            for (uint32_t x = 0; x < 4; ++x) {
#pragma unroll
                for (uint32_t y = 0; y < 4; ++y)
                    if (4 * x + y < nvalid) w[x] |= static_cast<uint32_t>(a.hay[q0 + 4 * x + y]) << (8 * y);
            }
        }
        if (a.gap == DAAC_GAP_CHARS) {
            uint32_t lead = 0;   // (c & 0xC0) != 0x80
#pragma unroll
            for (uint32_t x = 0; x < 4; ++x) {
                const uint32_t cont = w[x] & ~(w[x] << 1) & 0x80808080u;   // bit 7 of a byte: bit 7 set and bit 6 clear
#pragma unroll
                for (uint32_t y = 0; y < 4; ++y)
                    if (!((cont >> (8 * y + 7)) & 1u)) lead |= 1u << (4 * x + y);
            }
            rule = s.ends | lead;
        }
        s.w0 = w[0]; s.w1 = w[1]; s.w2 = w[2]; s.w3 = w[3];
    }
    s.flag = (s.mst | (~s.cov & rule)) & bits_below(nvalid);
    return s;
}

// the workgroup's exclusive prefix sum of v over its lanes (wave prefix sums by shuffles, the four wave totals through LDS) and its total
static __device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *s_wave, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t x = 0; x < kTokLanes / 64; ++x) {
        const uint32_t c = s_wave[x];
        if (x < wave) before += c;
        total += c;
    }
    __syncthreads();   // s_wave is written again in the next turn
    return before + inc - v;
}

__global__ __launch_bounds__(kTokLanes) void tokenize_count_kernel(const TokenizeArgs a) {
    __shared__ uint32_t s_wave[kTokLanes / 64];
    for (uint64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const TokLane s = tok_lane(a, t, a.gap == DAAC_GAP_CHARS);
        uint32_t total;
        (void)block_exclusive(__popc(s.flag), s_wave, total);
        if (threadIdx.x == 0) a.tile_cnt[t] = total;
    }
}

__global__ __launch_bounds__(kTokLanes) void tokenize_write_kernel(const TokenizeArgs a, const uint64_t n_tokens) {
    __shared__ uint32_t s_wave[kTokLanes / 64];
    for (uint64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const TokLane s = tok_lane(a, t, a.gap >= DAAC_GAP_BYTES);
        uint32_t total;
        const uint64_t rank0 = a.tile_cnt[t] + block_exclusive(__popc(s.flag), s_wave, total);
        if (!s.live) continue;
        const uint64_t q0 = s.q0;
        uint32_t ev = s.flag | s.ends;
        if (a.len - q0 < 16) ev |= 1u << static_cast<uint32_t>(a.len - q0);
        uint64_t i = s.j0, d = s.d0;
        uint64_t base = d ? doc_begin(a, d - 1) : 0;   // where the document of byte p - 1 begins
        while (ev) {
            const uint32_t b = __ffs(ev) - 1;
            ev &= ev - 1;
            const uint64_t p = q0 + b;
            const uint64_t rank = rank0 + __popc(s.flag & bits_below(b));
            const bool flagged = (s.flag >> b) & 1u;
            // here i = the number of matches with A_i < p: every one of them ended at an earlier event
            if (a.spans && a.gap != DAAC_GAP_SKIP && p > 0 && (flagged || p == a.len)) {
                const bool before_cov = b ? (s.cov >> (b - 1)) & 1u : s.prev_cov;
                if (!before_cov) {   // byte p - 1 is a gap token's last
                    const uint64_t idx = rank - 1 + (a.n_empty ? a.epre[i] : 0);
                    if (idx < n_tokens) a.spans[2 * idx + 1] = p - base;
                }
            }
            for (; d <= a.n_docs && doc_begin(a, d) == p; ++d) {
                if (a.tok_offsets) a.tok_offsets[d] = rank + (a.n_empty ? a.epre[a.doc_first[d]] : 0);
                base = p;
            }
            for (; i < a.k && a.aend[i] == p; ++i) {
                const uint4 m = a.seg[i];
                if (m.z) continue;
                const uint64_t idx = rank + a.epre[i];
                if (idx >= n_tokens) continue;
                a.ids[idx] = m.w;
                if (a.spans) { a.spans[2 * idx] = tok_seg_end(m); a.spans[2 * idx + 1] = tok_seg_end(m); }
            }
            if (!flagged) continue;
            const uint64_t idx = rank + (a.n_empty ? a.epre[i] : 0);
            if (idx >= n_tokens) continue;
            if ((s.mst >> b) & 1u) {   // match i begins here: the first that ends beyond p
                if (i >= a.k) continue;
                const uint4 m = a.seg[i];
                a.ids[idx] = m.w;
                if (a.spans) { a.spans[2 * idx] = tok_seg_end(m) - m.z; a.spans[2 * idx + 1] = tok_seg_end(m); }
            } else {
                a.ids[idx] = a.gap_id + (a.gap == DAAC_GAP_BYTES ? (lane_word(s, b >> 2) >> (8 * (b & 3))) & 0xffu : 0u);
                if (a.spans) a.spans[2 * idx] = p - base;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------- launchers
static uint32_t tok_grid(uint64_t items, uint64_t per_block, uint64_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_tokenize_prep(const TokenizeArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(tokenize_prep_kernel, dim3(tok_grid(a.k + 1, 256, 8192)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_tokenize_count(const TokenizeArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(tokenize_tiles_kernel, dim3(tok_grid(a.tiles + 1, 256, 8192)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tokenize_count_kernel, dim3(tok_grid(a.tiles, 1, kTokMaxBlocks)), dim3(kTokLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_tokenize_write(const TokenizeArgs &a, uint64_t n_tokens, hipStream_t stream) {
    hipLaunchKernelGGL(tokenize_write_kernel, dim3(tok_grid(a.tiles, 1, kTokMaxBlocks)), dim3(kTokLanes), 0, stream, a, n_tokens);
    return hipGetLastError();
}

}  // namespace daac
