// Per-pattern match counts of an overlapping scan (daac_scan_histogram) for gfx950.
//
// Every pattern has exactly one output record {value, length, parent} ("slot"), and a state's output list is the parent chain from
// its head record.  So the scan adds 1 at the HEAD slot of every hit and never walks a chain (hist_kernel: the segment scanners' loop of
// scan_kernels.hip — one lane per segment, entered `halo` bytes early from ROOT, hits with end in (lo, hi], ROOT's list at end 0 — with
// one no-return atomic per hit), hist_fold_kernel widens the 32-bit head counts into the caller's u64 array, and for find_overlapping
// hist_propagate_kernel pushes every head total down its parent links once.  Integer adds throughout: the result does not depend on
// the order they land in.
//
// Slots are numbered in BFS order of the trie, so the low slots are the short patterns — the ones that take most hits on natural text,
// and the addresses thousands of lanes would otherwise meet on in L2.  The first `lds_bins` slots are therefore counted per workgroup
// in LDS (behind the engine's tables) and flushed once at the workgroup's end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "hist.hpp"
#include "scan_engines.hpp"

namespace daac {

template <class Eng>
__global__ __launch_bounds__(1024) void hist_kernel(const typename Eng::Dev dev, const ScanArgs a, const HistArgs h) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Eng eng(dev, smem);
    eng.load_lds(smem);
    uint32_t *bins = reinterpret_cast<uint32_t *>(smem + h.off_bins);
    for (uint32_t i = threadIdx.x; i < h.lds_bins; i += blockDim.x) bins[i] = 0;
    __syncthreads();

    const uint8_t *__restrict__ hay = a.hay;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const uint32_t lds_bins = h.lds_bins, n = h.n;
    uint32_t *__restrict__ heads = h.heads;

    for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; seg < a.nseg; seg += stride) {
        const uint64_t lo = a.begin + seg * a.seg_bytes;
        const uint64_t hi = (lo + a.seg_bytes < a.len) ? lo + a.seg_bytes : a.len;
        uint64_t p = lo > a.halo ? lo - a.halo : 0;

        typename Eng::State st = eng.root();

        auto hit = [&](const typename Eng::State &s) {
            const uint32_t slot = eng.opos(s) - 1u;
            if (slot < lds_bins) __hip_atomic_fetch_add(bins + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if (slot < n) __hip_atomic_fetch_add(heads + slot, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };

        // ROOT's own list is drained once, at end = 0
        if (lo == 0 && eng.root_flag()) hit(st);

        for (; p < lo; ++p) eng.step(st, hay[p]);  // halo warm-up, nothing reported

        auto on_byte = [&](uint32_t c) {
            if (eng.step(st, c)) hit(st);
        };

        while (p < hi && (reinterpret_cast<uintptr_t>(hay + p) & 15u) != 0) on_byte(hay[p++]);
        const uint64_t nvec = (hi - p) >> 4;
        if (nvec != 0) {
            const uint8_t *vp = hay + p;
            u32x4_t cur = load_hay16(vp);
            for (uint64_t i = 0; i < nvec; ++i) {
                const u32x4_t nxt = load_hay16(vp + 16 * (i + 1 < nvec ? i + 1 : i));
                const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    on_byte(w[j] & 0xffu);
                    on_byte((w[j] >> 8) & 0xffu);
                    on_byte((w[j] >> 16) & 0xffu);
                    on_byte(w[j] >> 24);
                }
                cur = nxt;
            }
            p += nvec << 4;
        }
        while (p < hi) on_byte(hay[p++]);
    }

    __syncthreads();
    for (uint32_t i = threadIdx.x; i < lds_bins; i += blockDim.x) {
        const uint32_t v = bins[i];
        if (v != 0) __hip_atomic_fetch_add(heads + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void hist_fold_kernel(uint32_t *__restrict__ heads, unsigned long long *__restrict__ counts, uint64_t n) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint32_t v = heads[i];
        if (v != 0) { counts[i] += v; heads[i] = 0; }
    }
}

// `snap` is a copy of the head totals taken before this kernel runs: an ancestor receives each descendant's head total exactly once,
// whatever has already been added to counts[] by other lanes.
__global__ __launch_bounds__(256) void hist_propagate_kernel(const uint32_t *__restrict__ outputs, const unsigned long long *__restrict__ snap,
                                                             unsigned long long *__restrict__ counts, uint64_t n) {
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const unsigned long long v = snap[i];
        if (v == 0) continue;
        uint64_t at = i;
        for (;;) {
            const uint32_t parent = outputs[3 * at + 2];   // 1-based, 0 = none; parent - 1 < at: the walk ends
            if (parent == 0 || parent > at) break;
            at = parent - 1u;
            __hip_atomic_fetch_add(counts + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <class Eng>
static hipError_t launch_hist(const typename Eng::Dev &dev, const ScanArgs &a, const HistArgs &h, uint32_t blocks, uint32_t threads, uint32_t lds,
                              hipStream_t stream) {
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(hist_kernel<Eng>), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((hist_kernel<Eng>), dim3(blocks), dim3(threads), lds, stream, dev, a, h);
    return hipGetLastError();
}

hipError_t launch_hist_scan(const TierDev *tier, const DArrayDev *da, const CharDev *chr, const ScanArgs &a, const HistArgs &h, uint32_t blocks,
                            uint32_t threads, hipStream_t stream) {
    const uint32_t lds = std::max(16u, h.off_bins + 4u * h.lds_bins);
    if (lds > kHistLdsLimit || h.off_bins != hist_engine_lds(tier, da)) return hipErrorInvalidValue;
    if (tier) return tier->row32 ? launch_hist<TierEngine<true>>(*tier, a, h, blocks, threads, lds, stream)
                                 : launch_hist<TierEngine<false>>(*tier, a, h, blocks, threads, lds, stream);
    if (da) return launch_hist<DArrayEngine>(*da, a, h, blocks, threads, lds, stream);
    if (chr) return launch_hist<CharEngine>(*chr, a, h, blocks, threads, lds, stream);
    return hipErrorInvalidValue;
}

static uint32_t small_grid(uint64_t n) { return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(4096, (n + 255) / 256))); }

hipError_t launch_hist_fold(uint32_t *heads, unsigned long long *counts, uint64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(hist_fold_kernel, dim3(small_grid(n)), dim3(256), 0, stream, heads, counts, n);
    return hipGetLastError();
}

hipError_t launch_hist_propagate(const uint32_t *outputs, const unsigned long long *snap, unsigned long long *counts, uint64_t n, hipStream_t stream) {
    hipLaunchKernelGGL(hist_propagate_kernel, dim3(small_grid(n)), dim3(256), 0, stream, outputs, snap, counts, n);
    return hipGetLastError();
}

}  // namespace daac
