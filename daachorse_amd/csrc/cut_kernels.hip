// cut_batch and tokens_splice for gfx950 (daac_cut_batch, daac_tokens_splice).  cut.hpp has the definition, the layout and the
// per-lane bodies; this file has the kernels around them and their launchers.
//
//   cut count     one lane per item (a document, or one of its matches): the segments it contributes, 0, 1 or 2
//   cut write     the same lane writes its segments' starts and values at its rank; a document's item leaves its rank in doc_segs
//   splice count  one lane per segment: the tokens it gives the output
//   splice write  one wave per segment, its lanes over the segment's tokens: a text segment of thousands of tokens is not one lane's
//                 work, and the 64 lanes of a wave store 64 consecutive ids
//
// Every word is written by the one lane that owns it: vector stores, no atomics, no LDS.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cut.hpp"

namespace daac {

__global__ __launch_bounds__(kCutLanes) void cut_count_kernel(const CutArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x, items = a.n_docs + a.k;
    for (uint64_t x = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; x <= items; x += stride) a.counts[x] = cut_count_lane(a, x);
}

__global__ __launch_bounds__(kCutLanes) void cut_write_kernel(const CutArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x, items = a.n_docs + a.k;
    for (uint64_t x = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; x <= items; x += stride) cut_write_lane(a, x);
}

__global__ __launch_bounds__(kCutLanes) void splice_count_kernel(const SpliceArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; s <= a.n_segs; s += stride) a.out_seg_tok[s] = splice_count_lane(a, s);
}

__global__ __launch_bounds__(kCutLanes) void splice_write_kernel(const SpliceArgs a) {
    constexpr uint32_t kWaves = kCutLanes / 64;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWaves;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6); s < a.n_segs; s += stride) splice_write_segment(a, s, lane, 64u);
}

static uint32_t cut_grid(uint64_t lanes) {
    const uint64_t g = (lanes + kCutLanes - 1) / kCutLanes;
    return static_cast<uint32_t>(g < 1 ? 1 : g > kCutMaxBlocks ? kCutMaxBlocks : g);
}

hipError_t launch_cut_count(const CutArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(cut_count_kernel, dim3(cut_grid(a.n_docs + a.k + 1)), dim3(kCutLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cut_write(const CutArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(cut_write_kernel, dim3(cut_grid(a.n_docs + a.k + 1)), dim3(kCutLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_splice_count(const SpliceArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(splice_count_kernel, dim3(cut_grid(a.n_segs + 1)), dim3(kCutLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_splice_write(const SpliceArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(splice_write_kernel, dim3(cut_grid(a.n_segs * 64)), dim3(kCutLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace daac
