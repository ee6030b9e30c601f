// The charwise double array as the chain walkers (chain_scan.hpp) and the sync-point scanners want it: charwise_kernels.hip and
// batch_kernels.hip instantiate it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_scan.hpp"
#include "device_tables.hpp"

namespace daac {

struct CwState { uint32_t idx, base, fail, opos, filt; };  // filt (the child filter): only kept by the micro-step walker

// MAPLDS: ASCII and the populated stretch [map_lo, table_len) of the code mapper are staged in LDS as u16 (0xffff =
// unmapped): one L2 round trip less per character; the code points in between (rare in CJK text) go to the L2 copy
template <int LVL>  // what is staged in LDS: 0 nothing, 1 the code mapper, 2 the mapper and ROOT's row of children
struct CwTablesT {
    static constexpr bool MAPLDS = LVL >= 1, ROWLDS = LVL >= 2;
    using State = CwState;
    using Stream = HayStream;
    static constexpr bool kMicro = DAAC_CW_MICRO != 0;  // chain_scan.hpp: the walker takes the transition one memory round trip at a time
    const CharDev &d;
    uint4 root_rec;
    const uint8_t *__restrict__ hay;
    uint64_t len;  // real end of the haystack: nothing at or beyond it is read
    const uint16_t *l_map = nullptr;
    const uint2 *l_row = nullptr;  // CharDev::root_row in LDS

    // (word 3 of a walkers' record: output_pos | child filter << obits; the plain records have no filter bits)
    __device__ __forceinline__ uint32_t opos_of(uint32_t w) const { return d.fbits ? (w & ((1u << d.obits) - 1u)) : w; }
    __device__ __forceinline__ uint32_t filt_of(uint32_t w) const { return d.fbits ? (w >> d.obits) : 0xffffffffu; }
    __device__ __forceinline__ CwState root() const { return CwState{0, root_rec.x, root_rec.z, opos_of(root_rec.w), filt_of(root_rec.w)}; }
    // the automaton as chain_scan.hpp wants it
    // one scalar through the lane's haystack window (same decoding as scalar_at below)
    __device__ __forceinline__ uint32_t symbol_at(HayWindow &win, uint64_t pos, uint32_t &clen) const {
        const uint32_t b0 = win.byte_at(hay + pos);
        if (b0 < 0x80u) { clen = 1; return b0; }
        const uint32_t n = b0 < 0xe0u ? 2u : b0 < 0xf0u ? 3u : 4u;
        uint32_t cp = b0 < 0xe0u ? (b0 & 0x1fu) : b0 < 0xf0u ? (b0 & 0x0fu) : (b0 & 0x07u);
        for (uint32_t k = 1; k < n; ++k) cp = (cp << 6) | (pos + k < len ? (win.byte_at(hay + pos + k) & 0x3fu) : 0u);
        clen = n;
        return cp;
    }
    __device__ __forceinline__ uint32_t opos(const CwState &st) const { return st.opos; }
    __device__ __forceinline__ bool is_root(const CwState &st) const { return st.idx == 0; }
    __device__ __forceinline__ uint64_t boundary_at_or_after(uint64_t x) const {
        while (x < len && (hay[x] & 0xc0u) == 0x80u) ++x;
        return x;
    }

    // One scalar at byte `pos` (a character boundary of well-formed UTF-8; charwise/iter.rs:64-98).
    // A sequence cut by the end of the haystack is completed with zero payload bits, never read past.
    __device__ __forceinline__ uint32_t scalar_at(uint64_t pos, uint32_t &clen) const {
        const uint32_t b0 = hay[pos];
        if (b0 < 0x80u) { clen = 1; return b0; }
        const uint32_t n = b0 < 0xe0u ? 2u : b0 < 0xf0u ? 3u : 4u;
        uint32_t cp = b0 < 0xe0u ? (b0 & 0x1fu) : b0 < 0xf0u ? (b0 & 0x0fu) : (b0 & 0x07u);
        for (uint32_t k = 1; k < n; ++k) cp = (cp << 6) | (pos + k < len ? (hay[pos + k] & 0x3fu) : 0u);
        clen = n;
        return cp;
    }
    __device__ __forceinline__ uint32_t code_of(uint32_t cp) const {
        if (MAPLDS) {  // l_map: 128 entries for ASCII, then the stretch [map_lo, table_len)
            const uint32_t rel = cp - d.map_lo;
            const bool low = cp < 128u, high = rel < d.table_len - d.map_lo;
            if (low || high) {
                const uint32_t c = l_map[low ? cp : rel + 128u];
                return c == 0xffffu ? 0xffffffffu : c;
            }
            // between ASCII and the stretch: rare, from L2 — asked and waited for in one piece, so that the optimiser does
            // not, on the common path, wait for a load it would otherwise believe might be outstanding
            uint32_t c = 0xffffffffu;
            if (cp < d.table_len) asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(c) : "v"(d.table + cp) : "memory");
            return c;
        }
        return cp < d.table_len ? d.table[cp] : 0xffffffffu;
    }
    // The code of the scalar that begins at p (a character boundary of well-formed UTF-8; charwise/iter.rs:64-98) and its
    // length in bytes; `avail` bytes are left in the haystack: a sequence cut by its end is completed with zero payload bits.
    __device__ __forceinline__ uint32_t symbol_code(HayStream &win, uint32_t pos, uint32_t avail, uint32_t &clen) const {
        uint32_t x = win.word_at(pos);
        if (__builtin_amdgcn_ballot_w64(avail < 4u) != 0) {  // (only at the very end of the haystack: skipped by the whole wave otherwise)
            if (avail < 4u) x &= (1u << (8u * avail)) - 1u;
        }
        const uint32_t b0 = x & 0xffu;
        // one formula for the four lengths: the lead byte's payload over three 6-bit groups, shifted down by the groups not there
        const uint32_t m2 = b0 >= 0x80u, m3 = b0 >= 0xe0u, m4 = b0 >= 0xf0u;
        const uint32_t n = 1u + m2 + m3 + m4;
        const uint32_t lead = b0 & (0xffu >> (n + m2));  // 0x7f, 0x1f, 0x0f, 0x07
        const uint32_t tail = (((x >> 8) & 0x3fu) << 12) | (((x >> 16) & 0x3fu) << 6) | ((x >> 24) & 0x3fu);
        clen = n;
        return code_of(((lead << 18) | tail) >> (24u - 6u * n));
    }
    // One memory round trip of the transition on `code` (charwise.rs:1022-1050 / 1056-1092 taken apart): a probe of the child
    // slot, or — after a failed probe (phase 1), or at once when the state's child filter rules the child out — the record the
    // failure link leads to; a link to ROOT needs no memory (ROOT's row, or its record, is at hand), a DEAD link ends the walk.
    // True once the transition is complete.  Every lane loads, every turn (an idle lane asks for slot 0), and the outcome is a
    // handful of selects.
    template <bool LM>
    __device__ __forceinline__ bool micro(CwState &st, uint32_t code, uint32_t &phase, bool act) const {
        const bool known = act && code != 0xffffffffu;  // charwise.rs:1031-1035
        const bool at_root = st.idx == 0;
        const bool possible = st.base != 0 && ((st.filt >> (code & (d.fbits ? d.fbits - 1u : 0u))) & 1u) != 0;
        // with ROOT's row at hand a lane standing at ROOT asks memory nothing
        const bool probe = known && phase == 0 && possible && !(ROWLDS && at_root);
        const bool no_child = known && !probe;
        const bool stop = LM && st.fail == 1u;
        const bool follow = no_child && !at_root && !stop && st.fail != 0;
        const uint32_t slot = probe ? (st.base ^ code) : follow ? st.fail : 0u;
        uint2 e = uint2{2u << 30, 0u};
        if (ROWLDS) e = l_row[known ? code : 0u];
        // the turn's one memory round trip: all four words in one request, and the turn's one full wait with it
        typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
        U32x4 rv;
        asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(rv) : "v"(d.wstates + slot) : "memory");
        const uint4 r = uint4{rv.x, rv.y, rv.z, rv.w};
        uint32_t f = r.z;
        if (!LM && d.fail_plain) f = d.fail_plain[slot];
        const bool hit = probe && r.y == st.idx;
        const bool fell = no_child || (probe && !hit);             // no child on this symbol
        const bool take = hit || follow;                           // the record read becomes the state
        const bool dead = fell && !at_root && stop;
        const bool rootward = fell && !dead && (at_root || st.fail == 0);  // the symbol is ROOT's to take
        const bool by_row = ROWLDS && rootward;
        const bool child = by_row && (e.x >> 30) != 2u;
        const bool to_root = (act && !known) || dead || (rootward && !child);
        const bool done = (act && !known) || hit || dead || by_row || (fell && at_root);
        phase = (probe && !hit && !dead && !rootward) ? 1u : 0u;   // a failed probe whose link leads on: that record next turn
        const CwState rt = root();
        st.idx = take ? slot : child ? (rt.base ^ code) : to_root ? rt.idx : st.idx;
        st.base = take ? r.x : child ? (e.x & 0x3fffffffu) : to_root ? rt.base : st.base;
        st.fail = take ? f : child ? (e.x >> 30) : to_root ? rt.fail : st.fail;
        const uint32_t w = take ? r.w : e.y;
        st.opos = (take || child) ? opos_of(w) : to_root ? rt.opos : st.opos;
        st.filt = (take || child) ? filt_of(w) : to_root ? rt.filt : st.filt;
        return done;
    }
    __device__ __forceinline__ void load(CwState &st, uint32_t slot, bool plain) const {
        const uint4 r = d.states[slot];
        st = CwState{slot, r.x, (plain && d.fail_plain) ? d.fail_plain[slot] : r.z, r.w};
    }

    // classic delta: next_state_id_unchecked (charwise.rs:1022-1050) over links that never stop at DEAD
    __device__ __forceinline__ void step_plain(CwState &st, uint32_t cp) const {
        const uint32_t code = code_of(cp);
        if (code == 0xffffffffu) { st = root(); return; }
        for (;;) {
            if (st.base != 0) {
                const uint32_t child = st.base ^ code;
                const uint4 r = d.states[child];
                if (r.y == st.idx) { st = CwState{child, r.x, d.fail_plain ? d.fail_plain[child] : r.z, r.w}; return; }
            }
            if (st.idx == 0) return;
            load(st, st.fail, true);
        }
    }

    // next_state_id_leftmost_unchecked (charwise.rs:1056-1092): DEAD links end the walk at ROOT
    __device__ __forceinline__ void step_leftmost(CwState &st, uint32_t cp) const {
        const uint32_t code = code_of(cp);
        if (code == 0xffffffffu) { st = root(); return; }
        for (;;) {
            if (st.base != 0) {
                const uint32_t child = st.base ^ code;
                const uint4 r = d.states[child];
                if (r.y == st.idx) { st = CwState{child, r.x, r.z, r.w}; return; }
            }
            if (st.idx == 0) return;
            if (st.fail == 1u) { st = root(); return; }
            load(st, st.fail, false);
        }
    }

    // first sync point >= x
    __device__ __forceinline__ uint64_t sync_from(uint64_t x, uint32_t halo, uint64_t floor) const {
        if (x <= floor) return floor;  // the window start is a sync point by contract
        if (x >= len) return len;
        uint64_t pos = x > halo ? x - halo : 0;
        if (pos <= floor) pos = floor;
        else while (pos < len && (hay[pos] & 0xc0u) == 0x80u) ++pos;  // up to the next character boundary
        CwState st = root();
        uint32_t clen;
        while (pos < x) { const uint32_t cp = scalar_at(pos, clen); pos += clen; step_plain(st, cp); }
        while (st.idx != 0 && pos < len) { const uint32_t cp = scalar_at(pos, clen); pos += clen; step_plain(st, cp); }
        if (pos > len) pos = len;
        return st.idx == 0 ? pos : len;
    }
};
using CwTables = CwTablesT<0>;

}  // namespace daac
