// Restart scanners for gfx950: FindIterator (reference src/bytewise/iter.rs:58-113) and
// LeftmostFindIterator (iter.rs:272-340) on the device.
//
// Both iterators restart from ROOT after every match, so the scan is a chain through the match
// positions and cannot be cut at arbitrary offsets.  It CAN be cut at a *sync point*: a position p
// where the classic Aho-Corasick state of the text before p is ROOT, i.e. no pattern occurrence
// starts before p and ends after it.  Whatever the iterator did before p, at p it is at ROOT with
// nothing pending, and nothing it reports later starts before p — so the text from one sync point
// to the next can be scanned as if it were a haystack of its own.
//
// One lane per segment [lo, hi):
//   p = first sync point >= lo   (classic automaton warmed up over Lmax bytes — enough to land on the state a
//                                 lane that followed the text from further back is in, whatever its depth — then
//                                 advanced until it sits at ROOT); the lane owns nothing if p >= hi
//   q = first sync point >= hi   (same procedure) — the next owner starts exactly there
//   then the reference's loop, literally, over [p, q), positions offset by p.
// Regions [p, q) partition the haystack in order, so matches are placed by the same
// count -> exclusive scan -> write passes as the overlapping scan.  Text without sync points
// degrades gracefully: fewer, longer regions (in the limit one lane scans everything; still exact).
//
// Tables: the reference's double array, hot {base, opos_ch} / cold fail (DArrayDev); for leftmost
// automata the classic failure links are recomputed on the host (repack.cpp) next to the
// automaton's own (DEAD-terminated) ones.
#include <hip/hip_runtime.h>

#include <cstdint>

#define DAAC_RS_MICRO 1
#include "chain_scan.hpp"
#include "device_tables.hpp"
#include "restart_tables.hpp"

namespace daac {

__device__ __forceinline__ uint64_t rs_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}


// KMODE 0: totals {count, S1, S2}; 1: per-segment counts; 2: write matches at out + seg_counts[seg]
template <bool LEFTMOST, int KMODE>
__global__ __launch_bounds__(256) void restart_scan_kernel(const DArrayDev dev, const ScanArgs a, unsigned long long *next_begin) {
    __shared__ uint4 l_root[256];
    __shared__ unsigned long long scratch[3 * 4];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) l_root[i] = dev.root[i];
    __syncthreads();
    const RestartTables T{dev, l_root, a.hay};
    const uint8_t *__restrict__ hay = a.hay;
    const uint64_t len = a.total_len;  // real end of the haystack; a.len is the nominal end of this window
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    unsigned long long tot_cnt = 0;
    uint32_t tot_s1 = 0, tot_s2 = 0;

    for (uint64_t seg = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; seg < a.nseg; seg += stride) {
        const uint64_t lo = a.begin + seg * a.seg_bytes;
        const uint64_t hi = (lo + a.seg_bytes < a.len) ? lo + a.seg_bytes : a.len;
        const uint64_t p = T.sync_from(hay, lo, a.halo, a.begin, len);
        const bool last = hi == a.len;
        uint64_t q = 0;
        if (p < hi || last) q = T.sync_from(hay, hi, a.halo, a.begin, len);
        if (last && next_begin) *next_begin = q;  // where the next window (if any) has to start

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
                const uint32_t h = static_cast<uint32_t>(rs_mix64((static_cast<uint64_t>(value) << 32) | length));
                cnt += 1; s1 += h; s2 += h * static_cast<uint32_t>(end);
            }
        };

        if (!LEFTMOST && dev.root_flag) {
            // "" is a pattern: FindIterator degenerates to (p, p, first "" value) for every p
            // (iter.rs:60-85), whatever the text; positions (lo, hi] belong to this segment, 0 to the first
            const uint32_t op = dev.hot[0].y >> 8;
            if (lo == 0) emit(op, 0);
            for (uint64_t e = lo + 1; e <= hi; ++e) emit(op, e);
        } else if (p < hi || (LEFTMOST && last && p >= len && p == a.begin)) {  // (an empty range still ends the haystack)
            if (!LEFTMOST) {
                // FindIterator::next (iter.rs:87-112): restart at ROOT after every match, report the list head
                RsState st{0, 0, 0};
                for (uint64_t pos = p; pos < q; ++pos) {
                    T.step_plain(st, hay[pos]);
                    if ((st.opos_ch >> 8) != 0) {
                        emit(st.opos_ch >> 8, pos + 1);
                        st = RsState{0, 0, 0};
                    }
                }
            } else {
                // LeftmostFindIterator::next (iter.rs:272-340), call by call, over the bytes of [p, q).
                // `init` is ROOT's output_pos: non-zero when "" is a pattern, which then matches wherever no
                // longer match starts (iter.rs:254-261); every walk is then anchored at `pos` (all failure links
                // are DEAD) and has died by the sync point q.
                uint64_t pos = p;
                uint32_t init = dev.hot[0].y >> 8;
                bool skip_empty = false;
                const bool real_end = q >= len;
                for (;;) {                           // one pass = one call of next()
                    if (!real_end && pos >= q) break;  // the owner of the next region continues from q
                    RsState st{0, 0, 0};
                    uint32_t best = init;            // last_output_pos
                    const uint32_t init_at_entry = init;
                    // One emit site per path: hipcc 7.2 -O3 loses the advance of the output cursor when emit()
                    // is inlined behind the nested break/continue of the literal transcription.
                    uint32_t ret_op = 0;             // what this call returns, if the walk dies on a byte
                    uint64_t ret_end = 0;
                    bool again;
                    do {                             // the reference's loop 'a
                        again = false;
                        for (uint64_t i = pos; i < q; ++i) {
                            T.step_leftmost(st, hay[i]);
                            if (st.idx == 0) {
                                if (best != 0) {
                                    ret_end = pos;
                                    if (best != init) {
                                        skip_empty = true;
                                        ret_op = best;
                                    } else {
                                        pos += 1;
                                        if (skip_empty) { skip_empty = false; again = true; }
                                        else ret_op = best;
                                    }
                                    break;
                                }
                            } else if ((st.opos_ch >> 8) != 0) {
                                best = st.opos_ch >> 8;
                                pos = i + 1;
                            }
                        }
                    } while (again);
                    if (ret_op != 0) { emit(ret_op, ret_end); continue; }
                    // the bytes ran out (iter.rs:320-339)
                    if (!real_end) {                 // at a sync point only a match already seen can be pending
                        if (best != 0 && best != init_at_entry) { emit(best, pos); continue; }
                        break;
                    }
                    if (pos >= len) init = 0;
                    if (best == 0) break;            // None
                    if (best == init_at_entry && pos < len) {
                        // "" is a pattern and the haystack ends inside a longer one: the reference yields the same
                        // empty match forever from here (SURVEY 8a note D).  Reported, not imitated.
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

// ---- speculate / reconcile / emit (chain_scan.hpp) over the bytewise double array -------------------------
template <bool LEFTMOST, int PASS, int KMODE>
__global__ __launch_bounds__(256) void chain_kernel(const DArrayDev dev, const ScanArgs a, const ChainArgs c, unsigned long long *next_begin) {
    __shared__ uint4 l_root[256];
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(l_root);  // (used behind a barrier, when the walkers are through)
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) l_root[i] = dev.root_chain[i];
    __syncthreads();
    const RestartTables T{dev, l_root, a.hay};
    if (PASS == 0) chain_spec_body<RestartTables, LEFTMOST>(T, a, c, dev.ohash);
    else if (PASS == 1) chain_fix_body<RestartTables, LEFTMOST>(T, a, c, dev.ohash);
    else if (PASS == 3) chain_sum_body<KMODE>(a, c, next_begin, scratch);
    else chain_emit_body<RestartTables, LEFTMOST, KMODE>(T, a, c, dev.outputs, next_begin, scratch);
}

// find_overlapping_iter().count() (+ checksum) over the double array with the micro-step walker (chain_scan.hpp,
// overlap_count_body): the engine for automata the GRAM tables do not fit (more than 62 byte classes)
template <bool HEADS>
__global__ __launch_bounds__(256) void overlap_count_kernel(const DArrayDev dev, const ScanArgs a) {
    __shared__ uint4 l_root[256];
    unsigned long long *scratch = reinterpret_cast<unsigned long long *>(l_root);  // (used behind a barrier, when the walkers are through)
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) l_root[i] = dev.root_chain[i];
    __syncthreads();
    const RestartTables T{dev, l_root, a.hay};
    overlap_count_body<RestartTables, HEADS>(T, a, dev.osum, dev.ohash, scratch);
}

hipError_t launch_overlap_count(const DArrayDev &dev, const ScanArgs &a, bool heads, uint32_t blocks, hipStream_t stream) {
    if (heads) hipLaunchKernelGGL(overlap_count_kernel<true>, dim3(blocks), dim3(256), 0, stream, dev, a);
    else hipLaunchKernelGGL(overlap_count_kernel<false>, dim3(blocks), dim3(256), 0, stream, dev, a);
    return hipGetLastError();
}

hipError_t launch_chain(const DArrayDev &dev, const ScanArgs &a, const ChainArgs &c, int pass, int kmode, bool leftmost,
                        unsigned long long *next_begin, uint32_t blocks, hipStream_t stream) {
    const dim3 g(blocks), b(256);
#define DAAC_CH(L, P, M) hipLaunchKernelGGL((chain_kernel<L, P, M>), g, b, 0, stream, dev, a, c, next_begin)
    if (pass == 0) { if (leftmost) DAAC_CH(true, 0, 0); else DAAC_CH(false, 0, 0); }
    else if (pass == 1) { if (leftmost) DAAC_CH(true, 1, 0); else DAAC_CH(false, 1, 0); }
    else if (pass == 3) { if (kmode == 0) DAAC_CH(false, 3, 0); else DAAC_CH(false, 3, 1); }
    else if (leftmost) { if (kmode == 0) DAAC_CH(true, 2, 0); else if (kmode == 1) DAAC_CH(true, 2, 1); else DAAC_CH(true, 2, 2); }
    else { if (kmode == 0) DAAC_CH(false, 2, 0); else if (kmode == 1) DAAC_CH(false, 2, 1); else DAAC_CH(false, 2, 2); }
#undef DAAC_CH
    return hipGetLastError();
}

hipError_t launch_restart_scan(const DArrayDev &dev, const ScanArgs &a, int kmode, bool leftmost, unsigned long long *next_begin,
                               uint32_t blocks, uint32_t threads, hipStream_t stream) {
    const dim3 g(blocks), b(threads > 256 ? 256 : threads);
#define DAAC_RS(L, M) hipLaunchKernelGGL((restart_scan_kernel<L, M>), g, b, 0, stream, dev, a, next_begin)
    if (leftmost) { if (kmode == 0) DAAC_RS(true, 0); else if (kmode == 1) DAAC_RS(true, 1); else DAAC_RS(true, 2); }
    else { if (kmode == 0) DAAC_RS(false, 0); else if (kmode == 1) DAAC_RS(false, 1); else DAAC_RS(false, 2); }
#undef DAAC_RS
    return hipGetLastError();
}

}  // namespace daac
