// replace_all for gfx950 (daac_replace_all, daac_replace_all_batch): the passes between the tuple list and the spliced text.
//
//   size      one lane per match: which replacement it takes (and whether it has one), rlen_i and length_i for the two exclusive sums;
//             the tuple is rewritten in place as {end in the text, rlen, where the replacement lies in the blob}.
//   finish    O_i = end_i - L_{i+1} + R_i, the output position at which match i's replacement begins (non-decreasing in i).
//   tiles     one lane per tile of kSpliceTile output bytes: the last segment that begins at or before the tile's first byte.
//   splice    output-parallel: a workgroup owns a tile, a lane 16 bytes of it and one aligned 16-byte store.
//
// Output byte q belongs to the LARGEST i with O_i <= q ("segment i": match i's replacement, then the text up to the next match); before
// O_0 it is text, hay[q].  Any number of matches may share an output position — empty replacements, empty matches, adjacent matches —
// and all but the last of them contribute nothing at it: taking the largest i is what makes every tie right.
// Integer work only: the result is a function of the input alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "replace.hpp"

namespace daac {

static __device__ __forceinline__ uint64_t seg_end(const uint4 &t) { return static_cast<uint64_t>(t.x) | (static_cast<uint64_t>(t.y) << 32); }

__global__ __launch_bounds__(256) void replace_size_kernel(const ReplaceArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= a.k; i += stride) {
        if (i == a.k) { a.rpre[i] = 0; a.lpre[i] = 0; continue; }   // (the sums' entry k is the total)
        const uint4 t = a.seg[i];
        uint64_t end = seg_end(t);
        if (a.n_docs) {
            uint64_t lo = 0, hi = a.n_docs;  // the match's document: the last d with doc_first[d] <= i (doc_first[n_docs] = k > i, so it has matches)
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (a.doc_first[mid] <= i) lo = mid; else hi = mid;
            }
            end += a.doc_off[lo] - a.doc_off[0];
        }
        a.lpre[i] = t.z;
        const uint64_t r = a.n_repl == 1 ? 0 : t.w;
        if (r >= a.n_repl) {   // no replacement for this value: the tuple stays as it is for the driver's message
            atomicMin(a.bad, static_cast<unsigned long long>(i));
            a.rpre[i] = 0;
            continue;
        }
        const uint64_t at = a.roff[r], rlen = a.roff[r + 1] - at;
        a.rpre[i] = rlen;
        a.seg[i] = make_uint4(static_cast<uint32_t>(end), static_cast<uint32_t>(end >> 32), static_cast<uint32_t>(rlen), static_cast<uint32_t>(at));
    }
}

__global__ __launch_bounds__(256) void replace_doc_offsets_kernel(const ReplaceArgs a, unsigned long long *out_offsets) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride) {
        const uint64_t j = a.doc_first[d];   // every match before j lies in an earlier document
        out_offsets[d] = (a.doc_off[d] - a.doc_off[0]) - a.lpre[j] + a.rpre[j];
    }
}

__global__ __launch_bounds__(256) void replace_finish_kernel(const ReplaceArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.k; i += stride)
        a.rpre[i] = seg_end(a.seg[i]) - a.lpre[i + 1] + a.rpre[i];   // (lane i reads rpre[i] and lpre[i + 1] only: in place)
}

__global__ __launch_bounds__(256) void replace_tiles_kernel(const ReplaceArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t <= a.tiles; t += stride) {
        const uint64_t q = t * kSpliceTile;
        uint64_t lo = 0, hi = a.k;  // the number of segments that begin at or before q (entry `tiles`: q >= out_len >= every O_i, so all k)
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (a.rpre[mid] <= q) lo = mid + 1; else hi = mid;
        }
        a.tile_lo[t] = static_cast<long long>(lo) - 1;
    }
}

// The tile's segments after k_lo are numbered j = 0 .. m - 1 (segment k_lo + 1 + j); they begin inside the tile, at tile_begin + s_rel[j]
// when staged.  -> the first j in [lo, m] whose segment begins beyond q.
template <bool STAGED>
static __device__ __forceinline__ uint64_t segs_up_to(const uint32_t *s_rel, const unsigned long long *o_after, uint64_t tile_begin, uint64_t lo, uint64_t m,
                                                      uint64_t q) {
    uint64_t hi = m;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t p = STAGED ? tile_begin + s_rel[mid] : o_after[mid];
        if (p <= q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool STAGED>
static __device__ __forceinline__ void splice_lane(const ReplaceArgs &a, const uint32_t *s_rel, uint64_t tile_begin, long long k_lo, uint64_t m) {
    const uint64_t q0 = tile_begin + static_cast<uint64_t>(threadIdx.x) * 16;
    if (q0 >= a.out_len) return;
    const unsigned long long *o_after = a.rpre + (k_lo + 1);
    uint64_t j = segs_up_to<STAGED>(s_rel, o_after, tile_begin, 0, m, q0);   // the lane's first byte lies in segment k_lo + j
    // the segment in hand: it begins at output position o with rlen bytes of the blob from `at`, then text from `end`; the next begins at `next`
    uint64_t o, end, next;
    uint32_t rlen, at;
    auto fetch = [&]() {
        const long long s = k_lo + static_cast<long long>(j);
        if (s < 0) {   // before the first match: text from 0
            o = 0; end = 0; rlen = 0; at = 0;
        } else {
            const uint4 t = a.seg[s];
            o = a.rpre[s]; end = seg_end(t); rlen = t.z; at = t.w;
        }
        next = j < m ? (STAGED ? tile_begin + s_rel[j] : o_after[j]) : ~0ull;
    };
    fetch();
    const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(16, a.out_len - q0));
    if (n == 16 && q0 >= o + rlen && q0 + 16 <= next) {   // 16 bytes of one gap: the normal case on sparse text
        const uint64_t in = end + (q0 - o - rlen);
        if (in + 16 <= a.len) {
            uint4 v;
            __builtin_memcpy(&v, a.hay + in, 16);   // (any alignment)
            *reinterpret_cast<uint4 *>(a.out + q0) = v;
            return;
        }
    }
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t x = 0; x < 4; ++x) {
#pragma unroll
        for (uint32_t y = 0; y < 4; ++y) {
            const uint32_t b = 4 * x + y;
            if (b < n) {
                const uint64_t q = q0 + b;
                if (q >= next) {   // one step first; a binary search when more segments begin at or before q
                    ++j;
                    if (j < m && (STAGED ? tile_begin + s_rel[j] : o_after[j]) <= q) j = segs_up_to<STAGED>(s_rel, o_after, tile_begin, j + 1, m, q);
                    fetch();
                }
                const uint64_t d = q - o;
                uint32_t c = 0;   // (the two range checks hold by construction; a read outside either buffer must not happen whatever the lists say)
                if (d < rlen) { const uint64_t p = static_cast<uint64_t>(at) + d; if (p < a.repl_bytes) c = a.repl[p]; }
                else { const uint64_t p = end + (d - rlen); if (p < a.len) c = a.hay[p]; }
                w[x] |= c << (8 * y);
            }
        }
    }
    if (n == 16) {
        *reinterpret_cast<uint4 *>(a.out + q0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {   // the result's last granule
#pragma unroll
        for (uint32_t x = 0; x < 4; ++x) {
#pragma unroll
            for (uint32_t y = 0; y < 4; ++y)
                if (4 * x + y < n) a.out[q0 + 4 * x + y] = static_cast<uint8_t>(w[x] >> (8 * y));
        }
    }
}

__global__ __launch_bounds__(kSpliceLanes) void replace_splice_kernel(const ReplaceArgs a) {
    __shared__ uint32_t s_rel[kSpliceStage];
    for (uint64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const uint64_t tile_begin = t * kSpliceTile;
        const long long k_lo = a.tile_lo[t];
        // segments k_lo + 1 .. k_lo + m begin in (tile_begin, tile_begin + kSpliceTile]: the last value is never at or before a byte of the tile
        const uint64_t m = static_cast<uint64_t>(a.tile_lo[t + 1] - k_lo);
        if (m <= kSpliceStage) {   // (the same in every lane of the workgroup)
            for (uint64_t j = threadIdx.x; j < m; j += kSpliceLanes) s_rel[j] = static_cast<uint32_t>(a.rpre[k_lo + 1 + static_cast<long long>(j)] - tile_begin);
            __syncthreads();
            splice_lane<true>(a, s_rel, tile_begin, k_lo, m);
            __syncthreads();   // the next tile's positions go where these are still being read
        } else {
            splice_lane<false>(a, s_rel, tile_begin, k_lo, m);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- launchers
static uint32_t replace_grid(uint64_t items, uint64_t per_block, uint64_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_replace_size(const ReplaceArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(replace_size_kernel, dim3(replace_grid(a.k + 1, 256, 8192)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_replace_doc_offsets(const ReplaceArgs &a, unsigned long long *out_offsets, hipStream_t stream) {
    hipLaunchKernelGGL(replace_doc_offsets_kernel, dim3(replace_grid(a.n_docs + 1, 256, 4096)), dim3(256), 0, stream, a, out_offsets);
    return hipGetLastError();
}

hipError_t launch_replace_finish(const ReplaceArgs &a, hipStream_t stream) {
    if (a.k == 0) return hipSuccess;
    hipLaunchKernelGGL(replace_finish_kernel, dim3(replace_grid(a.k, 256, 8192)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_replace_splice(const ReplaceArgs &a, uint32_t num_cu, hipStream_t stream) {
    if (a.tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(replace_tiles_kernel, dim3(replace_grid(a.tiles + 1, 256, 8192)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(replace_splice_kernel, dim3(replace_grid(a.tiles, 1, static_cast<uint64_t>(std::max(1u, num_cu)) * 8)), dim3(kSpliceLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace daac
