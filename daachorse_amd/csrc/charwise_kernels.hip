// Restart scanners of the charwise automaton for gfx950: FindIterator (reference
// src/charwise/iter.rs:101-157) and LeftmostFindIterator (iter.rs:306-400) on the device.
//
// Same decomposition as restart_kernels.hip: the haystack is cut at *sync points* — character
// boundaries where the classic Aho-Corasick state of the text so far is ROOT — and the text
// between two sync points is scanned by one lane exactly as the reference scans a haystack of its
// own.  What differs from the bytewise file: symbols are UTF-8 scalars mapped to dense codes
// (charwise/mapper.rs), CHECK names the parent slot (charwise.rs:1022-1050), and positions move by
// whole characters while staying byte offsets.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_scan.hpp"
#include "device_tables.hpp"
#include "char_tables.hpp"

namespace daac {

__device__ __forceinline__ uint64_t cw_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}


// KMODE 0: totals {count, S1, S2}; 1: per-segment counts; 2: write matches at out + seg_counts[seg]
template <bool LEFTMOST, int KMODE>
__global__ __launch_bounds__(256) void char_restart_kernel(const CharDev dev, const ScanArgs a, unsigned long long *next_begin) {
    __shared__ unsigned long long scratch[3 * 4];
    const CwTables T{dev, dev.states[0], a.hay, a.total_len};
    const uint8_t *__restrict__ hay = a.hay;
    const uint64_t len = a.total_len;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned long long tot_cnt = 0;
    uint32_t tot_s1 = 0, tot_s2 = 0;

    for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; seg < a.nseg; seg += stride) {
        const uint64_t lo = a.begin + seg * a.seg_bytes;
        const uint64_t hi = (lo + a.seg_bytes < a.len) ? lo + a.seg_bytes : a.len;
        const bool positional = !LEFTMOST && dev.root_flag;
        uint64_t p = 0, q = 0;
        const bool final_seg = hi == a.len;
        if (!positional) {
            p = T.sync_from(lo, a.halo, a.begin);
            if (p < hi || final_seg) q = T.sync_from(hi, a.halo, a.begin);
        }
        if (final_seg && next_begin) *next_begin = positional ? hi : q;

        unsigned long long cnt = 0;
        uint32_t s1 = 0, s2 = 0;
        daac_match *o = nullptr;
        if (KMODE == 2) o = a.out + a.seg_counts[seg];
        auto emit = [&](uint32_t opos, uint64_t end) {
            const uint32_t *r = dev.outputs + 3u * (opos - 1u);
            const uint32_t value = r[0], length = r[1];
            if (KMODE == 2) {
                daac_match m;
                m.start = end - length; m.end = end; m.value = value; m._pad = 0;
                *o++ = m;
            } else {
                const uint32_t h = static_cast<uint32_t>(cw_mix64((static_cast<uint64_t>(value) << 32) | length));
                cnt += 1; s1 += h; s2 += h * static_cast<uint32_t>(end);
            }
        };

        if (positional) {
            // "" is a pattern: FindIterator reports (e, e, first "" value) at 0 and after every character
            // (iter.rs:115-131); ends in (lo, hi] belong to this segment
            const uint32_t op = T.root_rec.w;
            if (lo == 0) emit(op, 0);
            for (uint64_t e = lo + 1; e <= hi; ++e)
                if (e >= len || (hay[e] & 0xc0u) != 0x80u) emit(op, e);
        } else if (p < hi || (LEFTMOST && final_seg && p >= len && p == a.begin)) {  // (an empty range still ends the haystack)
            uint32_t clen;
            if (!LEFTMOST) {
                // FindIterator::next (iter.rs:133-156): back to ROOT after every match, report the list head
                CwState st = T.root();
                for (uint64_t pos = p; pos < q;) {
                    const uint32_t cp = T.scalar_at(pos, clen);
                    pos += clen;
                    T.step_plain(st, cp);
                    if (st.opos != 0) {
                        emit(st.opos, pos);
                        st = T.root();
                    }
                }
            } else {
                // LeftmostFindIterator::next (iter.rs:325-399), call by call, over the characters of [p, q).
                // `init` is the ROOT state's output_pos: non-zero when "" is a pattern, which then matches at
                // every position no longer match starts from (iter.rs:311-318); under that setting every walk
                // is anchored at `pos` (all failure links are DEAD) and has died by the sync point q.
                uint64_t pos = p;
                uint32_t init = T.root_rec.w;
                bool skip_empty = false;
                const bool real_end = q >= len;
                for (;;) {                       // one pass = one call of next()
                    if (!real_end && pos >= q) break;  // the owner of the next region continues from q
                    CwState st = T.root();
                    uint32_t best = init;        // last_output_pos
                    const uint32_t init_at_entry = init;
                    // One emit site per path: hipcc 7.2 -O3 loses the advance of the output cursor when emit() is
                    // inlined behind the nested break/continue of the literal transcription (seen in the ISA).
                    uint32_t ret_op = 0;         // what this call returns, if the walk dies on a character
                    uint64_t ret_end = 0;
                    bool again;
                    do {                         // the reference's loop 'a
                        again = false;
                        uint64_t i = pos, skips = 0;
                        while (i < q) {
                            const uint32_t cp = T.scalar_at(i, clen);
                            i += clen;
                            skips += clen;
                            T.step_leftmost(st, cp);
                            if (st.idx == 0) {
                                if (best != 0) {
                                    ret_end = pos;
                                    if (best != init) {
                                        skip_empty = true;
                                        ret_op = best;
                                    } else {
                                        pos += clen;
                                        if (skip_empty) { skip_empty = false; again = true; }
                                        else ret_op = best;
                                    }
                                    break;
                                }
                            } else if (st.opos != 0) {
                                best = st.opos;
                                pos += skips;
                                skips = 0;
                            }
                        }
                    } while (again);
                    if (ret_op != 0) { emit(ret_op, ret_end); continue; }
                    // the characters ran out (:385-398)
                    if (!real_end) {             // at a sync point only a match already seen can be pending
                        if (best != 0 && best != init_at_entry) { emit(best, pos); continue; }
                        break;
                    }
                    if (pos >= len) init = 0;
                    if (best == 0) break;        // None
                    if (best == init_at_entry && pos < len) {
                        // "" is a pattern and the haystack ends inside a longer one: the reference yields the
                        // same empty match forever from here (SURVEY 8a note D).  Reported, not imitated.
                        if (a.flags) atomicOr(a.flags, 1ull);
                        break;
                    }
                    emit(best, pos);
                }
            }
        }

        if (KMODE == 0) { tot_cnt += cnt; tot_s1 += s1; tot_s2 += s2; }
        else if (KMODE == 1) a.seg_counts[seg] = cnt;
    }

    if (KMODE == 0) {
        unsigned long long c = tot_cnt, x1 = tot_s1, x2 = tot_s2;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { c += __shfl_down(c, off, 64); x1 += __shfl_down(x1, off, 64); x2 += __shfl_down(x2, off, 64); }
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (lane == 0) { scratch[wave * 3] = c; scratch[wave * 3 + 1] = x1; scratch[wave * 3 + 2] = x2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long r0 = 0, r1 = 0, r2 = 0;
            for (int w = 0; w < static_cast<int>((blockDim.x + 63) >> 6); ++w) { r0 += scratch[w * 3]; r1 += scratch[w * 3 + 1]; r2 += scratch[w * 3 + 2]; }
            if (r0 | r1 | r2) { atomicAdd(a.result, r0); atomicAdd(a.result + 1, r1); atomicAdd(a.result + 2, r2); }
        }
    }
}

// ---- speculate / reconcile / emit (chain_scan.hpp) over the charwise double array -------------------------
template <bool LEFTMOST, int PASS, int KMODE, int LVL>
__global__ __launch_bounds__(LVL == 2 ? 1024 : LVL == 1 ? 512 : 256) void char_chain_kernel(const CharDev dev, const ScanArgs a, const ChainArgs c,
                                                                                           unsigned long long *next_begin) {
    extern __shared__ __attribute__((aligned(16))) uint16_t l_map[];
    __shared__ unsigned long long scratch[3 * 16];
    const uint32_t n_map = 128u + (dev.table_len - dev.map_lo);
    uint2 *l_row = reinterpret_cast<uint2 *>(reinterpret_cast<char *>(l_map) + ((n_map * 2u + 15u) & ~15u));
    if (LVL >= 1 && PASS != 3) {
        for (uint32_t i = threadIdx.x; i < n_map; i += blockDim.x) {
            const uint32_t cp = i < 128u ? i : i - 128u + dev.map_lo;
            const uint32_t code = cp < dev.table_len ? dev.table[cp] : 0xffffffffu;
            l_map[i] = code == 0xffffffffu ? 0xffffu : static_cast<uint16_t>(code);
        }
        if (LVL >= 2)
            for (uint32_t i = threadIdx.x; i < dev.alphabet; i += blockDim.x) l_row[i] = dev.root_row[i];
        __syncthreads();
    }
    const CwTablesT<LVL> T{dev, dev.wstates[0], a.hay, a.total_len, l_map, l_row};
    if (PASS == 0) chain_spec_body<CwTablesT<LVL>, LEFTMOST>(T, a, c, dev.ohash);
    else if (PASS == 1) chain_fix_body<CwTablesT<LVL>, LEFTMOST>(T, a, c, dev.ohash);
    else if (PASS == 3) chain_sum_body<KMODE>(a, c, next_begin, scratch);
    else chain_emit_body<CwTablesT<LVL>, LEFTMOST, KMODE>(T, a, c, dev.outputs, next_begin, scratch);
}

template <int LVL>
static hipError_t launch_char_chain_ml(const CharDev &dev, const ScanArgs &a, const ChainArgs &c, int pass, int kmode, bool leftmost,
                                       unsigned long long *next_begin, uint32_t blocks, hipStream_t stream) {
    // `blocks` counts 256-lane workgroups (8 per CU).  With the mapper in LDS (<= 32 KB) four 512-lane workgroups share a
    // CU, with ROOT's row as well (<= 80 KB together) two 1024-lane ones: the same 2048 lanes per CU every time.
    constexpr uint32_t per = LVL == 2 ? 4u : LVL == 1 ? 2u : 1u;
    const dim3 g((blocks + per - 1u) / per), b(256u * per);
    const uint32_t map_bytes = ((128u + dev.table_len - dev.map_lo) * 2u + 15u) & ~15u;
    const uint32_t lds = pass == 3 ? 0u : LVL == 2 ? map_bytes + dev.alphabet * 8u : LVL == 1 ? map_bytes : 0u;
    if (LVL == 2 && lds > 48u * 1024u) {
        hipError_t e;
#define DAAC_ATTR(L, P, M)                                                                                                      \
    do {                                                                                                                        \
        if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(char_chain_kernel<L, P, M, LVL>),                           \
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds))) != hipSuccess) return e; \
    } while (0)
        if (pass == 0) { if (leftmost) DAAC_ATTR(true, 0, 0); else DAAC_ATTR(false, 0, 0); }
        else if (pass == 1) { if (leftmost) DAAC_ATTR(true, 1, 0); else DAAC_ATTR(false, 1, 0); }
        else if (pass == 2 && leftmost) { if (kmode == 0) DAAC_ATTR(true, 2, 0); else if (kmode == 1) DAAC_ATTR(true, 2, 1); else DAAC_ATTR(true, 2, 2); }
        else if (pass == 2) { if (kmode == 0) DAAC_ATTR(false, 2, 0); else if (kmode == 1) DAAC_ATTR(false, 2, 1); else DAAC_ATTR(false, 2, 2); }
#undef DAAC_ATTR
    }
#define DAAC_CC(L, P, M) hipLaunchKernelGGL((char_chain_kernel<L, P, M, LVL>), g, b, lds, stream, dev, a, c, next_begin)
    if (pass == 0) { if (leftmost) DAAC_CC(true, 0, 0); else DAAC_CC(false, 0, 0); }
    else if (pass == 1) { if (leftmost) DAAC_CC(true, 1, 0); else DAAC_CC(false, 1, 0); }
    else if (pass == 3) { if (kmode == 0) DAAC_CC(false, 3, 0); else DAAC_CC(false, 3, 1); }
    else if (leftmost) { if (kmode == 0) DAAC_CC(true, 2, 0); else if (kmode == 1) DAAC_CC(true, 2, 1); else DAAC_CC(true, 2, 2); }
    else { if (kmode == 0) DAAC_CC(false, 2, 0); else if (kmode == 1) DAAC_CC(false, 2, 1); else DAAC_CC(false, 2, 2); }
#undef DAAC_CC
    return hipGetLastError();
}

// find_overlapping_iter().count() (+ checksum) of a charwise automaton with the micro-step walker (overlap_count_body)
template <int LVL, bool HEADS>
__global__ __launch_bounds__(LVL == 2 ? 1024 : LVL == 1 ? 512 : 256) void char_overlap_count_kernel(const CharDev dev, const ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t l_map[];
    __shared__ unsigned long long scratch[3 * 16];
    const uint32_t n_map = 128u + (dev.table_len - dev.map_lo);
    uint2 *l_row = reinterpret_cast<uint2 *>(reinterpret_cast<char *>(l_map) + ((n_map * 2u + 15u) & ~15u));
    if (LVL >= 1) {
        for (uint32_t i = threadIdx.x; i < n_map; i += blockDim.x) {
            const uint32_t cp = i < 128u ? i : i - 128u + dev.map_lo;
            const uint32_t code = cp < dev.table_len ? dev.table[cp] : 0xffffffffu;
            l_map[i] = code == 0xffffffffu ? 0xffffu : static_cast<uint16_t>(code);
        }
        if (LVL >= 2)
            for (uint32_t i = threadIdx.x; i < dev.alphabet; i += blockDim.x) l_row[i] = dev.root_row[i];
        __syncthreads();
    }
    const CwTablesT<LVL> T{dev, dev.wstates[0], a.hay, a.total_len, l_map, l_row};
    overlap_count_body<CwTablesT<LVL>, HEADS>(T, a, dev.osum, dev.ohash, scratch);
}

template <int LVL, bool HEADS>
static hipError_t launch_char_overlap_ml(const CharDev &dev, const ScanArgs &a, uint32_t blocks, hipStream_t stream) {
    constexpr uint32_t per = LVL == 2 ? 4u : LVL == 1 ? 2u : 1u;
    const dim3 g((blocks + per - 1u) / per), b(256u * per);
    const uint32_t map_bytes = ((128u + dev.table_len - dev.map_lo) * 2u + 15u) & ~15u;
    const uint32_t lds = LVL == 2 ? map_bytes + dev.alphabet * 8u : LVL == 1 ? map_bytes : 0u;
    if (lds > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(char_overlap_count_kernel<LVL, HEADS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((char_overlap_count_kernel<LVL, HEADS>), g, b, lds, stream, dev, a);
    return hipGetLastError();
}

// `blocks` counts 256-lane workgroups
hipError_t launch_char_overlap_count(const CharDev &dev, const ScanArgs &a, bool heads, uint32_t blocks, hipStream_t stream) {
    const int lvl = dev.map_in_lds != 0 ? (dev.row_in_lds != 0 ? 2 : 1) : 0;
    if (heads) return lvl == 2 ? launch_char_overlap_ml<2, true>(dev, a, blocks, stream) : lvl == 1 ? launch_char_overlap_ml<1, true>(dev, a, blocks, stream)
                                                                                                      : launch_char_overlap_ml<0, true>(dev, a, blocks, stream);
    return lvl == 2 ? launch_char_overlap_ml<2, false>(dev, a, blocks, stream) : lvl == 1 ? launch_char_overlap_ml<1, false>(dev, a, blocks, stream)
                                                                                           : launch_char_overlap_ml<0, false>(dev, a, blocks, stream);
}

hipError_t launch_char_chain(const CharDev &dev, const ScanArgs &a, const ChainArgs &c, int pass, int kmode, bool leftmost,
                             unsigned long long *next_begin, uint32_t blocks, hipStream_t stream) {
    if (dev.map_in_lds != 0 && dev.row_in_lds != 0) return launch_char_chain_ml<2>(dev, a, c, pass, kmode, leftmost, next_begin, blocks, stream);
    if (dev.map_in_lds != 0) return launch_char_chain_ml<1>(dev, a, c, pass, kmode, leftmost, next_begin, blocks, stream);
    return launch_char_chain_ml<0>(dev, a, c, pass, kmode, leftmost, next_begin, blocks, stream);
}

hipError_t launch_char_restart_scan(const CharDev &dev, const ScanArgs &a, int kmode, bool leftmost, unsigned long long *next_begin,
                                    uint32_t blocks, uint32_t threads, hipStream_t stream) {
    const dim3 g(blocks), b(threads > 256 ? 256 : threads);
#define DAAC_CW(L, M) hipLaunchKernelGGL((char_restart_kernel<L, M>), g, b, 0, stream, dev, a, next_begin)
    if (leftmost) { if (kmode == 0) DAAC_CW(true, 0); else if (kmode == 1) DAAC_CW(true, 1); else DAAC_CW(true, 2); }
    else { if (kmode == 0) DAAC_CW(false, 0); else if (kmode == 1) DAAC_CW(false, 1); else DAAC_CW(false, 2); }
#undef DAAC_CW
    return hipGetLastError();
}

}  // namespace daac
