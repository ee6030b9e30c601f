// HIP kernels of the daachorse scan path for gfx950 (MI355X / CDNA4).
//
// One wavefront lane scans one haystack segment.  A segment [lo, hi) is entered (Lmax - 1) bytes
// early from ROOT: the Aho-Corasick state after position p is a suffix of the text of length
// <= Lmax, so the halo reproduces the sequential state at `lo` exactly (SURVEY.md §8a note A) and
// the lane reports precisely the matches with end in (lo, hi], in the reference's order
// (FindOverlappingIterator::next, reference src/bytewise/iter.rs:133-176).  Concatenating the
// segments in order gives the reference stream; matches are placed by a count -> exclusive scan
// -> write pass, so the output is deterministic and needs no sorting.
//
// The transition function exists twice (see repack.hpp):
//   TierEngine   bitmap-rank trie, dense fail-resolved rows + child bitmaps in LDS
//   DArrayEngine the reference's double array (bytewise.rs:1063-1088), root row in LDS
// Integer work throughout; no MFMA.  The roofline of these kernels is HBM bytes of haystack.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_tables.hpp"
#include "scan_engines.hpp"

namespace daac {

// --------------------------------------------------------------------------------- the scan kernel
// MODE 0: count + checksum into a.result (atomics, one per workgroup)
// MODE 1: per-segment match counts into a.seg_counts
// MODE 2: write matches at a.out + a.seg_counts[seg] (exclusive offsets)
template <class Eng, int MODE, bool HEADS>
__global__ __launch_bounds__(1024) void scan_kernel(const typename Eng::Dev dev, const ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Eng eng(dev, smem);
    eng.load_lds(smem);
    __syncthreads();

    const uint8_t *__restrict__ hay = a.hay;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned long long tot_cnt = 0;
    uint32_t tot_s1 = 0, tot_s2 = 0;

    for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; seg < a.nseg; seg += stride) {
        const uint64_t lo = a.begin + seg * a.seg_bytes;
        const uint64_t hi = (lo + a.seg_bytes < a.len) ? lo + a.seg_bytes : a.len;
        uint64_t p = lo > a.halo ? lo - a.halo : 0;

        unsigned long long cnt = 0;
        uint32_t s1 = 0, s2 = 0, e = 0;  // e = end - lo of the byte just consumed
        daac_match *o = nullptr;
        if (MODE == 2) o = a.out + a.seg_counts[seg];

        typename Eng::State st = eng.root();

        auto emit = [&](const typename Eng::State &s) {
            if (MODE != 2) {
                if (HEADS) {  // FindOverlappingNoSuffixIterator: only the head of the list
                    const uint32_t *r = eng.outputs() + 3u * (eng.opos(s) - 1u);
                    const uint32_t h = match_hash32_dev(r[0], r[1]);
                    cnt += 1; s1 += h; s2 += h * e;
                } else {
                    const uint2 q = eng.sum(s);
                    cnt += q.x; s1 += q.y; s2 += q.y * e;
                }
            } else {
                uint32_t op = eng.opos(s);
                const uint64_t end = lo + e;
                do {
                    const uint32_t *r = eng.outputs() + 3u * (op - 1u);
                    const uint32_t value = r[0], length = r[1];
                    op = HEADS ? 0u : r[2];
                    daac_match m;
                    m.start = end - length; m.end = end; m.value = value; m._pad = 0;
                    *o++ = m;
                } while (op != 0);
            }
        };

        // ROOT's own list is drained once, at end = 0 (iter.rs:134-148 with pos = 0)
        if (lo == 0 && eng.root_flag()) emit(st);

        for (; p < lo; ++p) eng.step(st, hay[p]);  // halo warm-up, nothing reported

        auto on_byte = [&](uint32_t c) {
            ++e;
            if (eng.step(st, c)) emit(st);
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

        if (MODE == 0) {
            tot_cnt += cnt;
            tot_s1 += s1;
            tot_s2 += s2 + s1 * static_cast<uint32_t>(lo);  // sum h * low32(lo + e)
        } else if (MODE == 1) {
            a.seg_counts[seg] = cnt;
        }
    }

    if (MODE == 0) {
        unsigned long long c = wave_sum_u64(tot_cnt);
        unsigned long long x1 = wave_sum_u64(tot_s1);
        unsigned long long x2 = wave_sum_u64(tot_s2);
        __syncthreads();  // the tables in LDS are dead from here on
        unsigned long long *scratch = reinterpret_cast<unsigned long long *>(smem);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) { scratch[wave * 3 + 0] = c; scratch[wave * 3 + 1] = x1; scratch[wave * 3 + 2] = x2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int nw = (blockDim.x + 63) >> 6;
            unsigned long long r0 = 0, r1 = 0, r2 = 0;
            for (int w = 0; w < nw; ++w) { r0 += scratch[w * 3]; r1 += scratch[w * 3 + 1]; r2 += scratch[w * 3 + 2]; }
            if (r0 | r1 | r2) {
                atomicAdd(a.result + 0, r0);
                atomicAdd(a.result + 1, r1);
                atomicAdd(a.result + 2, r2);
            }
        }
    }
}

// Exclusive scan of per-segment counts (in place), total into result[0].  One workgroup:
// nseg is a few hundred thousand at most, this is microseconds.
__global__ __launch_bounds__(1024) void exclusive_scan_kernel(unsigned long long *v, uint64_t n, unsigned long long *total) {
    __shared__ unsigned long long part[1024];
    const uint64_t per = (n + blockDim.x - 1) / blockDim.x;
    const uint64_t b = per * threadIdx.x;
    const uint64_t e = b + per < n ? b + per : n;
    unsigned long long s = 0;
    for (uint64_t i = b; i < e; ++i) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (unsigned i = 0; i < blockDim.x; ++i) { const unsigned long long t = part[i]; part[i] = run; run += t; }
        *total = run;
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x];
    for (uint64_t i = b; i < e; ++i) { const unsigned long long t = v[i]; v[i] = run; run += t; }
}

// ------------------------------------------------------------------------------------- launchers
template <class Eng>
static hipError_t launch_mode(const typename Eng::Dev &dev, const ScanArgs &a, int mode, bool heads, dim3 grid, dim3 block,
                              uint32_t lds, hipStream_t stream) {
#define DAAC_LAUNCH(M, H) hipLaunchKernelGGL((scan_kernel<Eng, M, H>), grid, block, lds, stream, dev, a)
    if (mode == 0) { if (heads) DAAC_LAUNCH(0, true); else DAAC_LAUNCH(0, false); }
    else if (mode == 1) { if (heads) DAAC_LAUNCH(1, true); else DAAC_LAUNCH(1, false); }
    else { if (heads) DAAC_LAUNCH(2, true); else DAAC_LAUNCH(2, false); }
#undef DAAC_LAUNCH
    return hipGetLastError();
}

template <class K>
static hipError_t allow_lds(K kernel, uint32_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
}

hipError_t launch_tier_scan(const TierDev &dev, const ScanArgs &a, int mode, bool heads, uint32_t blocks, uint32_t threads,
                            hipStream_t stream) {
    const uint32_t lds = dev.lds_bytes;
    hipError_t e;
    if (dev.row32) {
        using E = TierEngine<true>;
        if ((e = allow_lds(scan_kernel<E, 0, false>, lds)) != hipSuccess) return e;
        if ((e = allow_lds(scan_kernel<E, 0, true>, lds)) != hipSuccess) return e;
        if ((e = allow_lds(scan_kernel<E, 1, false>, lds)) != hipSuccess) return e;
        if ((e = allow_lds(scan_kernel<E, 1, true>, lds)) != hipSuccess) return e;
        if ((e = allow_lds(scan_kernel<E, 2, false>, lds)) != hipSuccess) return e;
        if ((e = allow_lds(scan_kernel<E, 2, true>, lds)) != hipSuccess) return e;
        return launch_mode<E>(dev, a, mode, heads, dim3(blocks), dim3(threads), lds, stream);
    }
    using E = TierEngine<false>;
    if ((e = allow_lds(scan_kernel<E, 0, false>, lds)) != hipSuccess) return e;
    if ((e = allow_lds(scan_kernel<E, 0, true>, lds)) != hipSuccess) return e;
    if ((e = allow_lds(scan_kernel<E, 1, false>, lds)) != hipSuccess) return e;
    if ((e = allow_lds(scan_kernel<E, 1, true>, lds)) != hipSuccess) return e;
    if ((e = allow_lds(scan_kernel<E, 2, false>, lds)) != hipSuccess) return e;
    if ((e = allow_lds(scan_kernel<E, 2, true>, lds)) != hipSuccess) return e;
    return launch_mode<E>(dev, a, mode, heads, dim3(blocks), dim3(threads), lds, stream);
}

hipError_t launch_darray_scan(const DArrayDev &dev, const ScanArgs &a, int mode, bool heads, uint32_t blocks, uint32_t threads,
                              hipStream_t stream) {
    return launch_mode<DArrayEngine>(dev, a, mode, heads, dim3(blocks), dim3(threads), 256 * 16, stream);
}

hipError_t launch_char_scan(const CharDev &dev, const ScanArgs &a, int mode, bool heads, uint32_t blocks, uint32_t threads,
                            hipStream_t stream) {
    return launch_mode<CharEngine>(dev, a, mode, heads, dim3(blocks), dim3(threads), 1024, stream);
}

// The same for millions of counts (the tuple emitter: one per tile of 1 KiB of text), in three launches: sums of chunks of
// kScanChunk elements, their exclusive scan by the one-workgroup kernel above, the scan inside every chunk on top of its sum.
constexpr uint32_t kScanChunk = 2048;  // 256 threads x 8 consecutive elements
__global__ __launch_bounds__(256) void scan_chunk_sums_kernel(const unsigned long long *__restrict__ v, uint64_t n, unsigned long long *__restrict__ sums) {
    __shared__ unsigned long long part[4];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kScanChunk;
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint64_t i = base + static_cast<uint64_t>(k) * 256 + threadIdx.x;
        if (i < n) s += v[i];
    }
    s = wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
__global__ __launch_bounds__(256) void scan_chunks_kernel(unsigned long long *__restrict__ v, uint64_t n, const unsigned long long *__restrict__ sums_excl) {
    __shared__ unsigned long long part[256];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kScanChunk + static_cast<uint64_t>(threadIdx.x) * 8;
    unsigned long long x[8], s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { x[k] = base + k < n ? v[base + k] : 0ull; s += x[k]; }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < 64) {  // 256 thread sums: four per lane of the first wave
        unsigned long long q[4], t = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { q[k] = part[threadIdx.x * 4 + k]; t += q[k]; }
        unsigned long long incl = t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long y = __shfl_up(incl, off, 64);
            if (static_cast<int>(threadIdx.x) >= off) incl += y;
        }
        unsigned long long run = incl - t;
#pragma unroll
        for (int k = 0; k < 4; ++k) { part[threadIdx.x * 4 + k] = run; run += q[k]; }
    }
    __syncthreads();
    unsigned long long run = part[threadIdx.x] + sums_excl[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (base + k < n) v[base + k] = run;
        run += x[k];
    }
}

// `scratch`: room for n / kScanChunk + 2 more values (may be null for short arrays)
hipError_t launch_exclusive_scan(unsigned long long *v, uint64_t n, unsigned long long *total, unsigned long long *scratch, hipStream_t stream) {
    if (scratch == nullptr || n <= 4 * kScanChunk) {
        hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, v, n, total);
        return hipGetLastError();
    }
    const uint32_t nb = static_cast<uint32_t>((n + kScanChunk - 1) / kScanChunk);
    hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3(nb), dim3(256), 0, stream, v, n, scratch);
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, stream, scratch, static_cast<uint64_t>(nb), total);
    hipLaunchKernelGGL(scan_chunks_kernel, dim3(nb), dim3(256), 0, stream, v, n, scratch);
    return hipGetLastError();
}

}  // namespace daac
