// Per-document pattern counts of a batch for gfx950 (daac_scan_histogram_batch): the reduction of each document's slot records to
// rows {slot, count}, in ascending slot order.
//
// The record pass (batch_kernels.hip, MODE / KMODE 3) leaves document i's records — one 8-byte word per reported match, the slot in
// its low half — at rec[roff[i], roff[i+1]).  A document's distinct slots cannot outnumber its records, so its finished rows
// (slot | count << 32, 8 bytes as well) are written to the front of its own range; a last pass copies them to the CSR list.
// Three routes by the record count R of the document:
//   wave       R <= wave_max: one wave a document, four documents at a time per 256-lane workgroup.  The slots are sorted in the
//              wave's share of LDS (bitonic network, padded to a power of two with 0xFFFFFFFF — no slot has that number) and then
//              run-length encoded: a run's head finds its rank by ballot and its length by binary search for the run's end.
//   workgroup  R <= sort_max: the same with 1024 lanes a document and up to 128 KB of LDS; the head ranks go through per-wave totals.
//   dense      above: a row of u32 counters per document in HBM, added to with no-return atomics (integer adds: any order gives the
//              same row), then compacted in slot order by one workgroup a document.
// Every route's output is a function of the records as a multiset: nothing depends on the order in which lanes or atomics land.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "batch.hpp"

namespace daac {

constexpr uint32_t kPad = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void batch_hist_classify_kernel(const BatchHistArgs h, const unsigned long long *off, uint64_t max_len) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= h.n; i += stride) {
        if (i == h.n) { h.rowcnt[i] = 0; continue; }
        if (off[i + 1] - off[i] > max_len) atomicMin(h.cls + 2, static_cast<unsigned long long>(i));
        const uint64_t r = h.roff[i + 1] - h.roff[i];
        if (r <= h.wave_max) continue;
        if (r <= h.sort_max) h.group_list[atomicAdd(h.cls, 1ull)] = i;
        else h.dense_list[atomicAdd(h.cls + 1, 1ull)] = i;
    }
}

// A team is one wave (WAVE) or one workgroup.  Within a wave the LDS serves the wave's own accesses in program order, so a wave
// only has to keep the compiler from moving them across the point; a workgroup takes the barrier.
template <bool WAVE>
__device__ __forceinline__ void team_sync() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// rank of a flagged lane among the team's flagged lanes of this round, after `rows` earlier ones; `rows` advances by the round's total.
// Every lane of the team calls it (wtot: one word per wave of the workgroup).
template <bool WAVE>
__device__ __forceinline__ uint32_t team_rank(bool flag, uint32_t &rows, uint32_t *wtot) {
    const unsigned long long m = __ballot(flag);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
    uint32_t before = 0, all = static_cast<uint32_t>(__popcll(m));
    if (!WAVE) {
        const uint32_t w = threadIdx.x >> 6, nw = blockDim.x >> 6;
        if ((threadIdx.x & 63u) == 0) wtot[w] = all;
        __syncthreads();
        all = 0;
        for (uint32_t x = 0; x < nw; ++x) {
            const uint32_t v = wtot[x];
            before += x < w ? v : 0u;
            all += v;
        }
        __syncthreads();  // wtot is written again in the next round
    }
    const uint32_t rank = rows + before + below;
    rows += all;
    return rank;
}

// `cap`: slots of LDS per team (a power of two >= the route's largest R); the workgroup route keeps its wave totals behind them.
template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 256 : 1024) void batch_hist_sort_kernel(const BatchHistArgs h, uint64_t items, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hist_lds[];
    const uint32_t T = WAVE ? 64u : blockDim.x;
    const uint32_t t = WAVE ? (threadIdx.x & 63u) : threadIdx.x;
    uint32_t *s = WAVE ? hist_lds + (threadIdx.x >> 6) * cap : hist_lds;
    uint32_t *wtot = hist_lds + cap;  // (workgroup route only)
    const uint64_t team = WAVE ? static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6) : blockIdx.x;
    const uint64_t teams = WAVE ? static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6) : gridDim.x;
    for (uint64_t q = team; q < items; q += teams) {
        const uint64_t i = WAVE ? q : h.group_list[q];
        const uint64_t b = h.roff[i];
        const uint64_t r64 = h.roff[i + 1] - b;
        if (r64 > (WAVE ? h.wave_max : h.sort_max)) continue;  // another route's document (the whole team sees the same i)
        const uint32_t r = static_cast<uint32_t>(r64);
        if (r == 0) { if (t == 0) h.rowcnt[i] = 0; continue; }
        uint32_t p = 2;
        while (p < r) p <<= 1;  // p <= cap: r <= the route's limit <= cap
        unsigned long long *rec = h.rec + b;
        for (uint32_t k = t; k < p; k += T) s[k] = k < r ? static_cast<uint32_t>(rec[k]) : kPad;
        team_sync<WAVE>();
        for (uint32_t k = 2; k <= p; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t x = t; x < (p >> 1); x += T) {
                    const uint32_t lo = ((x & ~(j - 1u)) << 1) | (x & (j - 1u)), hi = lo | j;
                    const uint32_t a = s[lo], c = s[hi];
                    if ((a > c) == ((lo & k) == 0)) { s[lo] = c; s[hi] = a; }
                }
                team_sync<WAVE>();
            }
        }
        uint32_t rows = 0;
        for (uint32_t base = 0; base < r; base += T) {  // (r is the team's: every lane takes every round)
            const uint32_t k = base + t;
            const bool head = k < r && (k == 0 || s[k] != s[k - 1]);
            const uint32_t rank = team_rank<WAVE>(head, rows, wtot);
            if (head) {
                const uint32_t v = s[k];
                uint32_t lo = k + 1, hi = r;  // the run's end: the first position behind k whose slot is not v
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s[mid] == v) lo = mid + 1; else hi = mid;
                }
                rec[rank] = static_cast<unsigned long long>(v) | (static_cast<unsigned long long>(lo - k) << 32);
            }
        }
        if (t == 0) h.rowcnt[i] = rows;
        team_sync<WAVE>();  // the next document's slots go where this one's are still being read
    }
}

// dense route, 1: scratch[y][slot] += 1 for every record of document dense_list[d0 + y]
__global__ __launch_bounds__(256) void batch_hist_dense_add_kernel(const BatchHistArgs h, uint32_t *scratch, uint64_t slots, uint64_t d0) {
    const uint64_t i = h.dense_list[d0 + blockIdx.y];
    const uint64_t b = h.roff[i], r = h.roff[i + 1] - b;
    uint32_t *row = scratch + static_cast<uint64_t>(blockIdx.y) * slots;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < r; k += stride) {
        const uint32_t slot = static_cast<uint32_t>(h.rec[b + k]);
        if (slot < slots) atomicAdd(row + slot, 1u);  // (no value returned: the add is done at the L2)
    }
}

// dense route, 2: the non-zero counters of row blockIdx.x, in slot order, to the front of the document's record range
__global__ __launch_bounds__(1024) void batch_hist_dense_compact_kernel(const BatchHistArgs h, const uint32_t *scratch, uint64_t slots, uint64_t d0) {
    __shared__ uint32_t wtot[16];
    const uint64_t i = h.dense_list[d0 + blockIdx.x];
    unsigned long long *rec = h.rec + h.roff[i];
    const uint32_t *row = scratch + static_cast<uint64_t>(blockIdx.x) * slots;
    uint32_t rows = 0;
    for (uint64_t base = 0; base < slots; base += blockDim.x) {
        const uint64_t k = base + threadIdx.x;
        const uint32_t c = k < slots ? row[k] : 0u;
        const uint32_t rank = team_rank<false>(c != 0, rows, wtot);
        if (c != 0) rec[rank] = k | (static_cast<unsigned long long>(c) << 32);  // rank < the document's records: every counted slot has one
    }
    if (threadIdx.x == 0) h.rowcnt[i] = rows;
}

__global__ __launch_bounds__(256) void batch_hist_copy_kernel(const unsigned long long *rec, const unsigned long long *roff, const unsigned long long *doff,
                                                              uint64_t n, uint64_t total, unsigned long long *rows) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < total; r += stride) {
        uint64_t lo = 0, hi = n;  // the row's document: the last i with doff[i] <= r (doff[n] = total > r, so it has rows)
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (doff[mid] <= r) lo = mid; else hi = mid;
        }
        rows[r] = rec[roff[lo] + (r - doff[lo])];
    }
}

// ------------------------------------------------------------------------------------------------------- launchers
static uint32_t hist_grid(uint64_t items, uint64_t per_block, uint64_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

static uint32_t pow2_at_least(uint64_t v, uint32_t cap) {
    uint32_t p = 2;
    while (p < v && p < cap) p <<= 1;
    return p;
}

hipError_t launch_batch_hist_classify(const BatchHistArgs &h, const unsigned long long *off, uint64_t max_len, hipStream_t stream) {
    hipLaunchKernelGGL(batch_hist_classify_kernel, dim3(hist_grid(h.n + 1, 256, 4096)), dim3(256), 0, stream, h, off, max_len);
    return hipGetLastError();
}

hipError_t launch_batch_hist_sort(const BatchHistArgs &h, bool wave, uint64_t items, uint32_t num_cu, hipStream_t stream) {
    if (items == 0) return hipSuccess;
    if (wave) {
        const uint32_t cap = pow2_at_least(h.wave_max, kBatchHistWaveCap);
        const uint32_t lds = 4u * cap * sizeof(uint32_t);  // at most 64 KB
        const uint32_t bpc = std::max(1u, std::min(8u, (160u * 1024u) / lds));
        hipLaunchKernelGGL((batch_hist_sort_kernel<true>), dim3(hist_grid(items, 4, static_cast<uint64_t>(num_cu) * bpc)), dim3(256), lds, stream, h, items, cap);
        return hipGetLastError();
    }
    const uint32_t cap = pow2_at_least(h.sort_max, kBatchHistGroupCap);
    const uint32_t lds = (cap + 16u) * sizeof(uint32_t);
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(batch_hist_sort_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    const uint32_t bpc = std::max(1u, std::min(2u, (160u * 1024u) / lds));
    hipLaunchKernelGGL((batch_hist_sort_kernel<false>), dim3(hist_grid(items, 1, static_cast<uint64_t>(num_cu) * bpc)), dim3(1024), lds, stream, h, items, cap);
    return hipGetLastError();
}

hipError_t launch_batch_hist_dense(const BatchHistArgs &h, uint32_t *scratch, uint64_t slots, uint64_t d0, uint32_t nd, hipStream_t stream) {
    if (nd == 0) return hipSuccess;
    hipLaunchKernelGGL(batch_hist_dense_add_kernel, dim3(64, nd), dim3(256), 0, stream, h, scratch, slots, d0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(batch_hist_dense_compact_kernel, dim3(nd), dim3(1024), 0, stream, h, static_cast<const uint32_t *>(scratch), slots, d0);
    return hipGetLastError();
}

hipError_t launch_batch_hist_copy(const unsigned long long *rec, const unsigned long long *roff, const unsigned long long *doff, uint64_t n, uint64_t total,
                                  unsigned long long *rows, hipStream_t stream) {
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(batch_hist_copy_kernel, dim3(hist_grid(total, 256, 8192)), dim3(256), 0, stream, rec, roff, doff, n, total, rows);
    return hipGetLastError();
}

}  // namespace daac
