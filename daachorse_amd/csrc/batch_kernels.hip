// Batch scanners for gfx950: many independent documents in one call (daac_scan_count_batch / daac_scan_batch_device16).
//
// A batch is one buffer and n + 1 non-decreasing offsets; document i is [off[i], off[i+1]).  Every document is scanned as a
// haystack of its own: positions are relative to its first byte, nothing crosses its ends, ROOT's list is reported at its 0.
//
// Overlapping modes (find_overlapping_iter, find_overlapping_no_suffix_iter): the documents are cut into PIECES of at most
// `piece_bytes` (an empty document has one empty piece).  first_piece[] is the exclusive scan of pieces per document; a lane
// takes a piece, finds its document by binary search over first_piece[] and enters the piece min(halo, piece start - document
// start) bytes early at ROOT — the segment scanners' argument (scan_kernels.hip), with the document start as a hard floor.  The
// engines are those of the segment scanners (scan_engines.hpp).  MODE 0 leaves {count, S1, S2} per piece (ends relative to the
// document) and batch_reduce_kernel adds up each document's contiguous piece range; MODE 1 / 2 are the count -> exclusive scan
// -> write passes, writing daac_match16; MODE 3 is the write pass of daac_scan_histogram_batch: one 8-byte slot record per match.
//
// Chain modes (find_iter, leftmost_find_iter): one lane walks one whole document with ChainWalker (chain_scan.hpp) from its
// position 0 to its end; with "" in the set, find_iter reports every position and leftmost_find_iter runs the sync-point
// scanners' literal transcription of the reference loop (restart_kernels.hip / charwise_kernels.hip).  Documents longer than
// `lane_max` are skipped here; the host driver (api_batch.hip) sends them through the single-haystack path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "batch.hpp"
#include "char_tables.hpp"
#include "device_tables.hpp"
#include "restart_tables.hpp"
#include "scan_engines.hpp"

namespace daac {

// Validation of the offsets and pieces per document; pieces[n] = 0 so that the exclusive scan of n + 1 entries ends in the total.
__global__ __launch_bounds__(256) void batch_plan_kernel(const unsigned long long *off, uint64_t n, uint64_t piece_bytes, unsigned long long *pieces,
                                                         unsigned long long *flags) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += stride) {
        if (i == n) { if (pieces) pieces[n] = 0; continue; }
        const unsigned long long a = off[i], b = off[i + 1];
        if (b < a) atomicMin(flags, static_cast<unsigned long long>(i));
        const unsigned long long len = b > a ? b - a : 0;
        if (pieces) pieces[i] = len == 0 ? 1 : (len + piece_bytes - 1) / piece_bytes;
    }
}

// per document: the sum of {count, S1, S2} over [first[i], first[i+1]) (first == null: entry i alone) -> counts[i], checksums[i]
__global__ __launch_bounds__(256) void batch_reduce_kernel(const unsigned long long *first, const unsigned long long *res, uint64_t n,
                                                           unsigned long long *counts, unsigned long long *checksums) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t b = first ? first[i] : i, e = first ? first[i + 1] : i + 1;
        unsigned long long c = 0;
        uint32_t s1 = 0, s2 = 0;
        for (uint64_t j = b; j < e; ++j) {
            c += res[3 * j];
            s1 += static_cast<uint32_t>(res[3 * j + 1]);
            s2 += static_cast<uint32_t>(res[3 * j + 2]);
        }
        counts[i] = c;
        if (checksums) checksums[i] = (static_cast<unsigned long long>(s1) << 32) | s2;
    }
}

// CSR offsets per document from the exclusive offsets per piece: doc_off[i] = piece_off[first[i]], doc_off[n] = total
__global__ __launch_bounds__(256) void batch_doc_offsets_kernel(const unsigned long long *first, const unsigned long long *piece_off, uint64_t n,
                                                                const unsigned long long *total, unsigned long long *doc_off) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += stride)
        doc_off[i] = i == n ? *total : piece_off[first[i]];
}

// ------------------------------------------------------------------------------------------- overlapping modes, by piece
template <class Eng, int MODE, bool HEADS>
__global__ __launch_bounds__(1024) void batch_piece_kernel(const typename Eng::Dev dev, const BatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Eng eng(dev, smem);
    eng.load_lds(smem);
    __syncthreads();

    const uint8_t *__restrict__ hay = a.hay;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < a.npieces; j += stride) {
        // the document of piece j: the last i with first_piece[i] <= j (every document has a piece: the entries rise strictly)
        uint64_t lo_i = 0, hi_i = a.n;
        while (hi_i - lo_i > 1) {
            const uint64_t mid = (lo_i + hi_i) >> 1;
            if (a.first_piece[mid] <= j) lo_i = mid; else hi_i = mid;
        }
        const uint64_t doc = a.off[lo_i], doc_end = a.off[lo_i + 1];
        const uint64_t k = j - a.first_piece[lo_i];
        const uint64_t lo = doc + k * a.piece_bytes;
        const uint64_t hi = (lo + a.piece_bytes < doc_end) ? lo + a.piece_bytes : doc_end;
        const uint64_t rel = lo - doc;  // the piece's first position in document coordinates
        uint64_t p = lo - (rel < a.halo ? rel : a.halo);

        unsigned long long cnt = 0;
        uint32_t s1 = 0, s2 = 0, e = 0;  // e = end - lo of the byte just consumed
        uint4 *o = nullptr;
        unsigned long long *o8 = nullptr;
        if (MODE == 2) o = a.out + a.counts[j];
        if (MODE == 3) o8 = a.rec + a.counts[j];

        typename Eng::State st = eng.root();

        auto emit = [&](const typename Eng::State &s) {
            if (MODE < 2) {
                if (HEADS) {  // FindOverlappingNoSuffixIterator: only the head of the list
                    const uint32_t *r = eng.outputs() + 3u * (eng.opos(s) - 1u);
                    const uint32_t h = match_hash32_dev(r[0], r[1]);
                    cnt += 1; s1 += h; s2 += h * e;
                } else {
                    const uint2 q = eng.sum(s);
                    cnt += q.x; s1 += q.y; s2 += q.y * e;
                }
            } else if (MODE == 3) {  // the slot of every record of the list (HEADS: of its head)
                uint32_t op = eng.opos(s);
                do {
                    const uint32_t slot = op - 1u;
                    op = HEADS ? 0u : eng.outputs()[3u * slot + 2u];
                    *o8++ = slot;
                } while (op != 0);
            } else {
                uint32_t op = eng.opos(s);
                const uint64_t end = rel + e;
                do {
                    const uint32_t *r = eng.outputs() + 3u * (op - 1u);
                    const uint32_t value = r[0], length = r[1];
                    op = HEADS ? 0u : r[2];
                    *o++ = uint4{static_cast<uint32_t>(end), static_cast<uint32_t>(end >> 32), length, value};
                } while (op != 0);
            }
        };

        // ROOT's own list is drained once per document, at its end = 0
        if (k == 0 && eng.root_flag()) emit(st);

        for (; p < lo; ++p) eng.step(st, hay[p]);  // halo warm-up (never in front of the document), nothing reported

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
                for (int q = 0; q < 4; ++q) {
                    on_byte(w[q] & 0xffu);
                    on_byte((w[q] >> 8) & 0xffu);
                    on_byte((w[q] >> 16) & 0xffu);
                    on_byte(w[q] >> 24);
                }
                cur = nxt;
            }
            p += nvec << 4;
        }
        while (p < hi) on_byte(hay[p++]);

        if (MODE == 0) {
            a.res[3 * j] = cnt;
            a.res[3 * j + 1] = s1;
            a.res[3 * j + 2] = s2 + s1 * static_cast<uint32_t>(rel);  // sum h * low32(rel + e)
        } else if (MODE == 1) {
            a.counts[j] = cnt;
        }
    }
}

// ------------------------------------------------------------------------------------------- chain modes, by document
// LeftmostFindIterator::next with "" in the set, call by call over one whole document (the transcription of
// char_restart_kernel, with p = 0 and q = len: the document's end is the real end).  `sym(pos, clen)` reads one symbol.
// Returns false where the reference would not terminate (SURVEY 8a note D).
// (Not inlined: with the transcription inlined into the writing kernel, hipcc dropped an advance of the output cursor — the
// sync-point scanners met the same and keep one emit site per path.)
template <class T, class Sym, class Emit>
__device__ __attribute__((noinline)) bool leftmost_empty_doc(const T &t, uint64_t len, uint32_t init, Sym &&sym, Emit &&emit) {
    uint64_t pos = 0;
    bool skip_empty = false;
    uint32_t clen;
    for (;;) {                       // one pass = one call of next()
        typename T::State st = t.root();
        uint32_t best = init;        // last_output_pos
        const uint32_t init_at_entry = init;
        uint32_t ret_op = 0;         // what this call returns, if the walk dies on a symbol
        uint64_t ret_end = 0;
        bool again;
        do {                         // the reference's loop 'a
            again = false;
            uint64_t i = pos, skips = 0;
            while (i < len) {
                const uint32_t cp = sym(i, clen);
                i += clen;
                skips += clen;
                t.step_leftmost(st, cp);
                if (t.is_root(st)) {
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
                } else if (t.opos(st) != 0) {
                    best = t.opos(st);
                    pos += skips;
                    skips = 0;
                }
            }
        } while (again);
        if (ret_op != 0) { emit(ret_op, ret_end); continue; }
        if (pos >= len) init = 0;    // the symbols ran out
        if (best == 0) return true;  // None
        if (best == init_at_entry && pos < len) return false;
        emit(best, pos);
    }
}

// KMODE 0: {count, S1, S2} per document into res; 1: count per document; 2: write at out + counts[doc]; 3: slot records at
// rec + counts[doc].
// walk(h, len, emit) scans the document at h and returns false on note D.
template <int KMODE, class Walk>
__device__ __forceinline__ void batch_docs_body(const BatchArgs &a, const uint32_t *outputs, Walk &&walk) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const uint64_t doc = a.off[i], len = a.off[i + 1] - doc;
        if (len > a.lane_max) continue;  // the long route (host driver)
        unsigned long long cnt = 0;
        uint32_t s1 = 0, s2 = 0;
        uint4 *o = nullptr;
        unsigned long long *o8 = nullptr;
        if (KMODE == 2) o = a.out + a.counts[i];
        if (KMODE == 3) o8 = a.rec + a.counts[i];
        auto emit = [&](uint32_t opos, uint64_t end) {
            const uint32_t *r = outputs + 3u * (opos - 1u);
            const uint32_t value = r[0], length = r[1];
            if (KMODE == 3) {
                o8[cnt] = opos - 1u;
            } else if (KMODE == 2) {
                o[cnt] = uint4{static_cast<uint32_t>(end), static_cast<uint32_t>(end >> 32), length, value};
            } else {
                const uint32_t h = match_hash32_dev(value, length);
                s1 += h; s2 += h * static_cast<uint32_t>(end);
            }
            cnt += 1;
        };
        if (!walk(a.hay + doc, len, emit)) atomicMin(a.flags + 1, static_cast<unsigned long long>(i));
        if (KMODE == 0) { a.res[3 * i] = cnt; a.res[3 * i + 1] = s1; a.res[3 * i + 2] = s2; }
        else if (KMODE == 1) a.counts[i] = cnt;
    }
}

constexpr uint64_t kNoCap = 1ull << 40;  // a walk over a whole document never runs past its `hi`

template <bool LEFTMOST, int KMODE>
__global__ __launch_bounds__(256) void batch_chain_kernel(const DArrayDev dev, const BatchArgs a) {
    __shared__ uint4 l_chain[256];  // ROOT's row as the chain walkers want it
    __shared__ uint4 l_root[256];   // ... and as the sync-point scanners' transitions want it
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) { l_chain[i] = dev.root_chain[i]; l_root[i] = dev.root[i]; }
    __syncthreads();
    const uint32_t init = dev.hot[0].y >> 8;  // ROOT's output_pos: "" is a pattern
    batch_docs_body<KMODE>(a, dev.outputs, [&](const uint8_t *h, uint64_t len, auto &emit) -> bool {
        if (dev.root_flag && !LEFTMOST) {  // FindIterator reports (p, p, first "" value) for every p (iter.rs:60-85)
            for (uint64_t e = 0; e <= len; ++e) emit(init, e);
            return true;
        }
        if (dev.root_flag) {
            const RestartTables T{dev, l_root, h};
            return leftmost_empty_doc(T, len, init, [&](uint64_t pos, uint32_t &clen) -> uint32_t { clen = 1; return h[pos]; }, emit);
        }
        const RestartTables T{dev, l_chain, h};
        ChainWalker<RestartTables, LEFTMOST> w{T, len, kNoCap};
        w.run(0, len, emit);
        return true;
    });
}

template <bool LEFTMOST, int KMODE>
__global__ __launch_bounds__(256) void batch_char_chain_kernel(const CharDev dev, const BatchArgs a) {
    batch_docs_body<KMODE>(a, dev.outputs, [&](const uint8_t *h, uint64_t len, auto &emit) -> bool {
        if (dev.root_flag && !LEFTMOST) {  // FindIterator reports "" at 0 and after every character (charwise/iter.rs:115-131)
            const uint32_t op = dev.states[0].w;
            for (uint64_t e = 0; e <= len; ++e)
                if (e == 0 || e >= len || (h[e] & 0xc0u) != 0x80u) emit(op, e);
            return true;
        }
        if (dev.root_flag) {
            const CwTables T{dev, dev.states[0], h, len};
            return leftmost_empty_doc(T, len, T.root_rec.w, [&](uint64_t pos, uint32_t &clen) -> uint32_t { return T.scalar_at(pos, clen); }, emit);
        }
        const CwTables T{dev, dev.wstates[0], h, len};
        ChainWalker<CwTables, LEFTMOST> w{T, len, kNoCap};
        w.run(0, len, emit);
        return true;
    });
}

// ------------------------------------------------------------------------------------------------------- launchers
static uint32_t grid_for(uint64_t items, uint32_t threads, uint32_t cap) {
    const uint64_t g = (items + threads - 1) / threads;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_batch_plan(const unsigned long long *off, uint64_t n, uint64_t piece_bytes, unsigned long long *pieces, unsigned long long *flags,
                             hipStream_t stream) {
    hipLaunchKernelGGL(batch_plan_kernel, dim3(grid_for(n + 1, 256, 4096)), dim3(256), 0, stream, off, n, piece_bytes, pieces, flags);
    return hipGetLastError();
}

hipError_t launch_batch_reduce(const unsigned long long *first, const unsigned long long *res, uint64_t n, unsigned long long *counts,
                               unsigned long long *checksums, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(batch_reduce_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, stream, first, res, n, counts, checksums);
    return hipGetLastError();
}

hipError_t launch_batch_doc_offsets(const unsigned long long *first, const unsigned long long *piece_off, uint64_t n, const unsigned long long *total,
                                    unsigned long long *doc_off, hipStream_t stream) {
    hipLaunchKernelGGL(batch_doc_offsets_kernel, dim3(grid_for(n + 1, 256, 4096)), dim3(256), 0, stream, first, piece_off, n, total, doc_off);
    return hipGetLastError();
}

template <class Eng>
static hipError_t launch_pieces_eng(const typename Eng::Dev &dev, const BatchArgs &a, int mode, bool heads, uint32_t blocks, uint32_t threads,
                                    uint32_t lds, hipStream_t stream) {
#define DAAC_BP(M, H)                                                                                                                   \
    do {                                                                                                                                \
        if (lds > 64 * 1024) {                                                                                                          \
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(batch_piece_kernel<Eng, M, H>),                     \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));                \
            if (e != hipSuccess) return e;                                                                                              \
        }                                                                                                                               \
        hipLaunchKernelGGL((batch_piece_kernel<Eng, M, H>), dim3(blocks), dim3(threads), lds, stream, dev, a);                         \
    } while (0)
    if (mode == 0) { if (heads) DAAC_BP(0, true); else DAAC_BP(0, false); }
    else if (mode == 1) { if (heads) DAAC_BP(1, true); else DAAC_BP(1, false); }
    else if (mode == 2) { if (heads) DAAC_BP(2, true); else DAAC_BP(2, false); }
    else { if (heads) DAAC_BP(3, true); else DAAC_BP(3, false); }
#undef DAAC_BP
    return hipGetLastError();
}

// exactly one of tier / da / chr: as many workgroups per CU as the LDS allows (two 1024-lane ones at most)
hipError_t launch_batch_pieces(const TierDev *tier, const DArrayDev *da, const CharDev *chr, const BatchArgs &a, int mode, bool heads, uint32_t num_cu,
                               uint32_t threads, hipStream_t stream) {
    const uint32_t lds = tier ? tier->lds_bytes : da ? 256u * 16u : 1024u;
    const uint32_t bpc = std::max(1u, std::min(2048u / threads, (160u * 1024u) / std::max(lds, 1u)));
    const uint32_t blocks = grid_for(a.npieces, threads, num_cu * bpc);
    if (tier) {
        return tier->row32 ? launch_pieces_eng<TierEngine<true>>(*tier, a, mode, heads, blocks, threads, lds, stream)
                           : launch_pieces_eng<TierEngine<false>>(*tier, a, mode, heads, blocks, threads, lds, stream);
    }
    if (da) return launch_pieces_eng<DArrayEngine>(*da, a, mode, heads, blocks, threads, lds, stream);
    return launch_pieces_eng<CharEngine>(*chr, a, mode, heads, blocks, threads, lds, stream);
}

hipError_t launch_batch_chain(const DArrayDev *da, const CharDev *chr, const BatchArgs &a, int kmode, bool leftmost, uint32_t num_cu, hipStream_t stream) {
    const dim3 g(grid_for(a.n, 256, num_cu * 8)), b(256);
#define DAAC_BC(K, L, M) hipLaunchKernelGGL((K<L, M>), g, b, 0, stream, *dev, a)
    if (da) {
        const DArrayDev *dev = da;
        if (leftmost) { if (kmode == 0) DAAC_BC(batch_chain_kernel, true, 0); else if (kmode == 1) DAAC_BC(batch_chain_kernel, true, 1); else if (kmode == 2) DAAC_BC(batch_chain_kernel, true, 2); else DAAC_BC(batch_chain_kernel, true, 3); }
        else { if (kmode == 0) DAAC_BC(batch_chain_kernel, false, 0); else if (kmode == 1) DAAC_BC(batch_chain_kernel, false, 1); else if (kmode == 2) DAAC_BC(batch_chain_kernel, false, 2); else DAAC_BC(batch_chain_kernel, false, 3); }
    } else {
        const CharDev *dev = chr;
        if (leftmost) { if (kmode == 0) DAAC_BC(batch_char_chain_kernel, true, 0); else if (kmode == 1) DAAC_BC(batch_char_chain_kernel, true, 1); else if (kmode == 2) DAAC_BC(batch_char_chain_kernel, true, 2); else DAAC_BC(batch_char_chain_kernel, true, 3); }
        else { if (kmode == 0) DAAC_BC(batch_char_chain_kernel, false, 0); else if (kmode == 1) DAAC_BC(batch_char_chain_kernel, false, 1); else if (kmode == 2) DAAC_BC(batch_char_chain_kernel, false, 2); else DAAC_BC(batch_char_chain_kernel, false, 3); }
    }
#undef DAAC_BC
    return hipGetLastError();
}

}  // namespace daac
