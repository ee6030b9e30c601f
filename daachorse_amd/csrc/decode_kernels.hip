// tokens_decode for gfx950 (daac_tokens_decode).  decode.hpp has the definition, the layout and the per-lane bodies; this file has the
// kernels around them and their launchers.
//
//   size     one lane per token: the rest image's length (0: not kept, or in no document) and a cleared mark.  A lane keeps the lowest
//            token without an entry (as the max of the complement) and the kept tokens of what it strode over; a wave folds its 64
//            lanes' values with xor shuffles and lane 0 adds them to the call's words: one atomic per wave and word, on scratch
//   header   one lane per document: the token range checked, the first kept token's length and mark overridden; the first document in
//            error folded the same way
//   offsets  one lane per document, behind the sum: out_offsets
//   tiles    one lane per tile of kDecodeTile output bytes: the last token that begins at or before the tile's first byte
//   copy     output-parallel: a workgroup owns a tile, a lane 16 bytes of it and one aligned 16-byte store; the starts of the tile's
//            tokens in LDS where there are at most kDecodeStage of them
// Integer work only: the result is a function of the input alone.  No pass uses atomics on the output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "decode.hpp"

namespace daac {

template <class Op>
static __device__ __forceinline__ unsigned long long decode_wave_fold(unsigned long long v, Op op) {
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(kDecodeSizeLanes) void decode_size_kernel(const DecodeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    uint64_t lo, hi;
    decode_span(a, lo, hi);
    unsigned long long unknown = 0, kept = 0;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= a.n_tokens; i += stride) {
        if (i == a.n_tokens) {   // the closing entry: the sum's total
            a.start[i] = 0;
            break;
        }
        const DecodeSized r = decode_size_lane(a, i, lo, hi);
        kept += r.kept;
        if (r.unknown) {
            const unsigned long long code = ~static_cast<unsigned long long>(i);   // the lowest index has the largest
            unknown = code > unknown ? code : unknown;
        }
    }
    // every lane of the wave is here: the loop above leaves to this point only
    unknown = decode_wave_fold(unknown, [](unsigned long long x, unsigned long long y) { return x > y ? x : y; });
    kept = decode_wave_fold(kept, [](unsigned long long x, unsigned long long y) { return x + y; });
    if ((threadIdx.x & 63u) == 0) {
        if (unknown) atomicMax(a.fold + 1, unknown);
        if (kept) atomicAdd(a.fold + 2, kept);
    }
}

__global__ __launch_bounds__(kDecodeSizeLanes) void decode_header_kernel(const DecodeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned long long err = 0;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d < a.n_docs; d += stride) {
        if (!decode_header_lane(a, d)) {
            const unsigned long long code = ~static_cast<unsigned long long>(d);   // the first document in error has the largest
            err = code > err ? code : err;
        }
    }
    err = decode_wave_fold(err, [](unsigned long long x, unsigned long long y) { return x > y ? x : y; });
    if ((threadIdx.x & 63u) == 0 && err) atomicMax(a.fold + 0, err);
}

__global__ __launch_bounds__(kDecodeSizeLanes) void decode_doc_offsets_kernel(const DecodeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride) decode_doc_offset_lane(a, d);
}

__global__ __launch_bounds__(kDecodeSizeLanes) void decode_tiles_kernel(const DecodeArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t <= a.tiles; t += stride) decode_tile_lane(a, t);
}

__global__ __launch_bounds__(kDecodeLanes) void decode_copy_kernel(const DecodeArgs a) {
    __shared__ uint16_t s_rel[kDecodeStage];   // (an offset of 1 .. kDecodeTile)
    for (uint64_t t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const uint64_t tile_begin = t * kDecodeTile;
        long long k_lo;
        const uint64_t m = decode_tile_tokens(a, t, k_lo);
        if (m <= kDecodeStage) {   // (the same in every lane of the workgroup)
            for (uint64_t j = threadIdx.x; j < m; j += kDecodeLanes) s_rel[j] = static_cast<uint16_t>(a.start[k_lo + 1 + static_cast<long long>(j)] - tile_begin);
            __syncthreads();
            decode_copy_lane<true>(a, s_rel, tile_begin, k_lo, m, threadIdx.x);
            __syncthreads();   // the next tile's positions go where these are still being read
        } else {
            decode_copy_lane<false>(a, s_rel, tile_begin, k_lo, m, threadIdx.x);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- launchers
static uint32_t decode_grid(uint64_t items, uint64_t per_block, uint64_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_decode_size(const DecodeArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(decode_size_kernel, dim3(decode_grid(a.n_tokens + 1, kDecodeSizeLanes, kDecodeMaxBlocks)), dim3(kDecodeSizeLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_decode_header(const DecodeArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(decode_header_kernel, dim3(decode_grid(a.n_docs, kDecodeSizeLanes, kDecodeMaxBlocks)), dim3(kDecodeSizeLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_decode_doc_offsets(const DecodeArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(decode_doc_offsets_kernel, dim3(decode_grid(a.n_docs + 1, kDecodeSizeLanes, kDecodeMaxBlocks)), dim3(kDecodeSizeLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_decode_copy(const DecodeArgs &a, uint32_t num_cu, hipStream_t stream) {
    if (a.tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(decode_tiles_kernel, dim3(decode_grid(a.tiles + 1, kDecodeSizeLanes, 8192)), dim3(kDecodeSizeLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(decode_copy_kernel, dim3(decode_grid(a.tiles, 1, static_cast<uint64_t>(std::max(1u, num_cu)) * 8)), dim3(kDecodeLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace daac
