// The transition engines of the segment scanners (scan_kernels.hip) and of the batch scanners (batch_kernels.hip): one lane
// feeds an engine bytes and reports the output list of every state it enters.  See scan_kernels.hip for how they are used.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "device_tables.hpp"

namespace daac {

// ------------------------------------------------------------------------------------------ utils
__device__ __forceinline__ uint64_t mix64_dev(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t match_hash32_dev(uint32_t value, uint32_t length) {
    return static_cast<uint32_t>(mix64_dev((static_cast<uint64_t>(value) << 32) | length));
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Streaming (non-temporal) 16-byte haystack load: the haystack is read once and must not evict
// the automaton tables from L2.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4_t load_hay16(const uint8_t *p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
}

// Cooperative global -> LDS copy of a table (16-byte granules; sizes are padded by the host).
__device__ __forceinline__ void copy_to_lds(void *dst, const void *src, uint32_t bytes) {
    const uint4 *s = reinterpret_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    for (uint32_t i = threadIdx.x; i < bytes / 16; i += blockDim.x) d[i] = s[i];
}

// ------------------------------------------------------------------------------------ TierEngine
template <bool ROW32>
struct TierEngine {
    using Dev = TierDev;
    using Row = typename std::conditional<ROW32, uint32_t, uint16_t>::type;
    struct State { uint32_t id; };

    const TierDev &d;
    const Row *l_rows;
    const uint32_t *l_bcmap;
    const uint32_t *l_bfail;
    const uint2 *l_ssum;
    const uint8_t *l_cls;

    __device__ TierEngine(const TierDev &dev, char *smem)
        : d(dev),
          l_rows(reinterpret_cast<const Row *>(smem)),
          l_bcmap(reinterpret_cast<const uint32_t *>(smem + dev.off_bcmap)),
          l_bfail(reinterpret_cast<const uint32_t *>(smem + dev.off_bfail)),
          l_ssum(reinterpret_cast<const uint2 *>(smem + dev.off_ssum)),
          l_cls(reinterpret_cast<const uint8_t *>(smem + dev.off_cls)) {}

    __device__ void load_lds(char *smem) const {
        copy_to_lds(smem, d.rows, d.off_bcmap);
        copy_to_lds(smem + d.off_bcmap, d.bcmap, d.off_bfail - d.off_bcmap);
        copy_to_lds(smem + d.off_bfail, d.bfail, d.off_ssum - d.off_bfail);
        copy_to_lds(smem + d.off_ssum, d.ssum, d.off_cls - d.off_ssum);
        copy_to_lds(smem + d.off_cls, d.cls, 256);
    }

    __device__ __forceinline__ State root() const { return State{0}; }
    __device__ __forceinline__ bool root_flag() const { return d.root_flag != 0; }

    // delta(state, byte) -> new state; returns whether the new state carries an output list.
    __device__ __forceinline__ bool step(State &st, uint32_t c) const {
        const uint32_t k = l_cls[c];
        uint32_t s = st.id;
        for (;;) {
            if (s < d.NA) {  // tier A: dense row, failure links already resolved
                const uint32_t e = l_rows[s * d.C + k];
                constexpr uint32_t kShift = ROW32 ? 31 : 15;
                st.id = e & ((1u << kShift) - 1u);
                return (e >> kShift) != 0;
            }
            uint32_t cmap, omap, first, fail;
            if (s < d.NB) {  // tier B: bitmap and fail in LDS, the rest only on a hit
                cmap = l_bcmap[s - d.NA];
                if (((cmap >> k) & 1u) == 0) { s = l_bfail[s - d.NA]; continue; }
                const uint4 r = d.grec[s];
                omap = r.y; first = r.z;
            } else {         // tier C: one 16-byte record from L2/HBM
                const uint4 r = d.grec[s];
                cmap = r.x; omap = r.y; first = r.z; fail = r.w;
                if (((cmap >> k) & 1u) == 0) { s = fail; continue; }
            }
            st.id = first + __popc(cmap & ((1u << k) - 1u));
            return ((omap >> k) & 1u) != 0;
        }
    }

    // {number of outputs, sum of their h32} of the state's output list
    __device__ __forceinline__ uint2 sum(const State &st) const {
        return st.id < d.NA ? l_ssum[st.id] : d.ssum[st.id];
    }
    __device__ __forceinline__ uint32_t opos(const State &st) const { return d.sopos[st.id]; }
    __device__ __forceinline__ const uint32_t *outputs() const { return d.outputs; }
};

// ---------------------------------------------------------------------------------- DArrayEngine
struct DArrayEngine {
    using Dev = DArrayDev;
    struct State { uint32_t idx, base, opos_ch; };

    const DArrayDev &d;
    const uint4 *l_root;

    __device__ DArrayEngine(const DArrayDev &dev, char *smem) : d(dev), l_root(reinterpret_cast<const uint4 *>(smem)) {}
    __device__ void load_lds(char *smem) const { copy_to_lds(smem, d.root, 256 * 16); }

    __device__ __forceinline__ State root() const {
        const uint2 h = d.hot[0];
        return State{0, h.x, h.y};
    }
    __device__ __forceinline__ bool root_flag() const { return d.root_flag != 0; }

    // next_state_id_unchecked, reference src/bytewise.rs:1063-1088
    __device__ __forceinline__ bool step(State &st, uint32_t c) const {
        for (;;) {
            if (st.idx == 0) {
                const uint4 r = l_root[c];  // {child, child.base, child.opos_ch}
                st = State{r.x, r.y, r.z};
                return (r.z >> 8) != 0;
            }
            if (st.base != 0) {
                const uint32_t child = st.base ^ c;
                const uint2 h = d.hot[child];
                if ((h.y & 0xffu) == c) {
                    st = State{child, h.x, h.y};
                    return (h.y >> 8) != 0;
                }
            }
            const uint32_t f = d.fail[st.idx];
            if (f == 0) { st.idx = 0; continue; }
            const uint2 h = d.hot[f];
            st = State{f, h.x, h.y};
        }
    }

    __device__ __forceinline__ uint2 sum(const State &st) const { return d.osum[(st.opos_ch >> 8) - 1]; }
    __device__ __forceinline__ uint32_t opos(const State &st) const { return st.opos_ch >> 8; }
    __device__ __forceinline__ const uint32_t *outputs() const { return d.outputs; }
};

// ------------------------------------------------------------------------------------ CharEngine
// CharwiseDoubleArrayAhoCorasick (reference src/charwise.rs:1022-1050): the lane is fed bytes and
// assembles UTF-8 scalars itself (charwise/iter.rs:64-98); a transition happens when a scalar is
// complete, so `e` in the scan loop is the byte offset of the END of the character, which is what
// the reference reports.  A segment may begin or end inside a character: continuation bytes seen
// before the first lead byte are skipped, and a character cut by the segment end is finished by
// the next lane (its halo starts earlier).  Unmapped scalars send the automaton to ROOT.
struct CharEngine {
    using Dev = CharDev;
    struct State { uint32_t idx, base, fail, opos, cp, need; };

    const CharDev &d;
    uint4 root_rec;

    __device__ CharEngine(const CharDev &dev, char *) : d(dev), root_rec(dev.states[0]) {}
    __device__ void load_lds(char *) const {}

    __device__ __forceinline__ State root() const { return State{0, root_rec.x, root_rec.z, root_rec.w, 0, 0}; }
    __device__ __forceinline__ bool root_flag() const { return d.root_flag != 0; }

    __device__ __forceinline__ bool step(State &st, uint32_t b) const {
        if (b < 0x80u) { st.cp = b; st.need = 0; }
        else if (b < 0xc0u) {
            if (st.need == 0) return false;  // inside a character that began before the lane's first byte
            st.cp = (st.cp << 6) | (b & 0x3fu);
            if (--st.need != 0) return false;
        } else {
            st.cp = b < 0xe0u ? (b & 0x1fu) : b < 0xf0u ? (b & 0x0fu) : (b & 0x07u);
            st.need = b < 0xe0u ? 1u : b < 0xf0u ? 2u : 3u;
            return false;
        }
        const uint32_t code = st.cp < d.table_len ? d.table[st.cp] : 0xffffffffu;
        if (code == 0xffffffffu) {  // charwise.rs:1031-1035
            st.idx = 0; st.base = root_rec.x; st.fail = root_rec.z; st.opos = root_rec.w;
            return root_rec.w != 0;
        }
        for (;;) {
            if (st.base != 0) {
                const uint32_t child = st.base ^ code;
                const uint4 r = d.states[child];
                if (r.y == st.idx) {
                    st.idx = child; st.base = r.x; st.fail = r.z; st.opos = r.w;
                    return r.w != 0;
                }
            }
            if (st.idx == 0) return root_rec.w != 0;
            const uint32_t f = st.fail;
            const uint4 r = d.states[f];
            st.idx = f; st.base = r.x; st.fail = r.z; st.opos = r.w;
        }
    }

    __device__ __forceinline__ uint2 sum(const State &st) const { return d.osum[st.opos - 1]; }
    __device__ __forceinline__ uint32_t opos(const State &st) const { return st.opos; }
    __device__ __forceinline__ const uint32_t *outputs() const { return d.outputs; }
};

}  // namespace daac
