// tokens_pack for gfx950 (daac_tokens_pack).  pack.hpp has the definition, the layout and the per-lane bodies; this file has the two
// kernels around them and their launchers.
//
//   header  one lane per document: what A and B keep and where, the row's length.  A lane keeps the longest row, the first document in
//           error, the slots and the dropped tokens of the documents it strode over; a wave folds its 64 lanes' values with xor
//           shuffles and lane 0 adds them to the call's four words: one atomic per wave and word
//   slots   one lane per output slot of the flat n * L (or R) index space: a wave's 64 lanes store 64 consecutive elements of every
//           plane (512 bytes of an int64 plane, 1 KiB of the offsets), whatever the rows' lengths; every word is written by the one
//           lane that owns it: vector stores, no atomics, no LDS
//
// The launch shape of both is pack_grid below: kPackLanes lanes a workgroup, at most kPackMaxBlocks workgroups, which stride.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pack.hpp"

namespace daac {

template <class Op>
__device__ __forceinline__ unsigned long long wave_fold(unsigned long long v, Op op) {
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(kPackLanes) void pack_header_kernel(const PackArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint64_t first = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long longest = 0, err = 0, slots = 0, dropped = 0;
    for (uint64_t d = first; d <= a.n_docs; d += stride) {
        if (d == a.n_docs) {   // the closing entry
            if (a.row_len) a.row_len[d] = 0;
            break;
        }
        const PackRow r = pack_header_lane(a, d);
        longest = r.row_len > longest ? r.row_len : longest;
        slots += r.row_len;
        dropped += r.dropped;
        if (r.error) {
            const unsigned long long code = ~(2ull * d + r.why);   // the first document in error has the largest
            err = code > err ? code : err;
        }
    }
    // every lane of the wave is here: the loop above leaves to this point only
    const auto mx = [](unsigned long long x, unsigned long long y) { return x > y ? x : y; };
    const auto add = [](unsigned long long x, unsigned long long y) { return x + y; };
    longest = wave_fold(longest, mx);
    err = wave_fold(err, mx);
    slots = wave_fold(slots, add);
    dropped = wave_fold(dropped, add);
    if ((threadIdx.x & 63u) == 0) {
        if (longest) atomicMax(a.fold + 0, longest);
        if (err) atomicMax(a.fold + 1, err);
        if (slots) atomicAdd(a.fold + 2, slots);
        if (dropped) atomicAdd(a.fold + 3, dropped);
    }
}

__global__ __launch_bounds__(kPackLanes) void pack_slots_kernel(const PackArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t x = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; x < a.slots; x += stride) pack_slot_lane(a, x);
}

static uint32_t pack_grid(uint64_t lanes) {
    const uint64_t g = (lanes + kPackLanes - 1) / kPackLanes;
    return static_cast<uint32_t>(g < 1 ? 1 : g > kPackMaxBlocks ? kPackMaxBlocks : g);
}

hipError_t launch_pack_header(const PackArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(pack_header_kernel, dim3(pack_grid(a.n_docs + 1)), dim3(kPackLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_pack_slots(const PackArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(pack_slots_kernel, dim3(pack_grid(a.slots)), dim3(kPackLanes), 0, stream, a);
    return hipGetLastError();
}

}  // namespace daac
