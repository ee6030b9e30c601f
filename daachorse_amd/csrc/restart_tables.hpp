// The bytewise double array as the chain walkers (chain_scan.hpp) and the sync-point scanners want it: restart_kernels.hip and
// batch_kernels.hip instantiate it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#ifndef DAAC_RS_MICRO
#define DAAC_RS_MICRO 1
#endif
#include "chain_scan.hpp"
#include "device_tables.hpp"

namespace daac {

struct RsState { uint32_t idx, base, opos_ch, fail, fmap; };  // fail, fmap (the child filter): only kept by the micro-step walker (chain_scan.hpp, run_micro)

struct RestartTables {
    using State = RsState;
    static constexpr bool kMicro = DAAC_RS_MICRO != 0;  // chain_scan.hpp: the walker takes the transition one memory round trip at a time
    const DArrayDev &d;
    const uint4 *l_root;  // in LDS: 256 x {child, child.base, child.opos_ch, child.fail} (restart_scan_kernel), or DArrayDev::root_chain (the walkers)
    const uint8_t *__restrict__ hay = nullptr;
    using Stream = HayStream;

    // the automaton as chain_scan.hpp wants it
    __device__ __forceinline__ RsState root() const { return RsState{0, 0, 0}; }
    __device__ __forceinline__ uint32_t symbol_at(HayWindow &win, uint64_t pos, uint32_t &clen) const { clen = 1; return win.byte_at(hay + pos); }
    __device__ __forceinline__ uint32_t opos(const RsState &st) const { return st.opos_ch >> 8; }
    __device__ __forceinline__ bool is_root(const RsState &st) const { return st.idx == 0; }
    __device__ __forceinline__ uint64_t boundary_at_or_after(uint64_t x) const { return x; }

    // ---- the micro-step walker's view (chain_scan.hpp, run_micro) ----
    __device__ __forceinline__ uint32_t symbol_code(Stream &win, uint32_t pos, uint32_t, uint32_t &clen) const {
        clen = 1;
        return win.byte_at(pos);
    }
    // One memory round trip of the transition on byte c (bytewise.rs:1063-1088 / 1094-1128 taken apart) over the 16-byte
    // records {base, opos_ch, fail, child filter}: phase 0 probes the child slot, phase 1 fetches the record a failure link
    // leads to.  ROOT's row is in LDS: a lane at ROOT, or one whose failed probe leaves it with a link to ROOT, is through
    // without asking memory — and so is a probe the state's child filter rules out (no child on any byte with these low five
    // bits): a failed probe lands on an arbitrary element of the array, i.e. on a cache line nobody else wants, and on text
    // that leaves the dictionary's words after three or four bytes those were most of the walkers' misses.  Every lane loads,
    // every turn (an idle lane asks for slot 0); the outcome is a handful of selects.
    template <bool LM>
    __device__ __forceinline__ bool micro(RsState &st, uint32_t c, uint32_t &phase, bool act) const {
        const bool at_root = st.idx == 0;
        const bool child_possible = st.base != 0 && ((st.fmap >> (c & 31u)) & 1u) != 0;
        // what this turn asks memory: the child slot (a probe), or — after a failed probe (phase 1), or at once when the filter
        // rules the child out — the record the failure link leads to, unless that link ends the walk (DEAD) or leads to ROOT
        const bool probe = act && phase == 0 && !at_root && child_possible;
        const bool no_child = act && !at_root && !probe;
        const bool stop = LM && st.fail == 1u;          // the link is DEAD: the walk ends
        const bool follow = no_child && !stop && st.fail != 0;
        const uint32_t slot = probe ? (st.base ^ c) : follow ? st.fail : 0u;
        const uint4 rr = l_root[c];
        typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));
        U32x4 r;
        asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(d.rec + slot) : "memory");
        const bool hit = probe && (r.y & 0xffu) == c;
        const bool miss = probe && !hit;
        const bool dead = (no_child || miss) && stop;
        const bool rootward = act && !dead && (at_root || ((no_child || miss) && st.fail == 0));
        const bool take = hit || follow;
        phase = (miss && !dead && !rootward) ? 1u : 0u;   // a failed probe whose link leads on: that record next turn
        st.idx = take ? slot : rootward ? rr.x : dead ? 0u : st.idx;
        st.base = take ? r.x : rootward ? rr.y : dead ? 0u : st.base;
        st.opos_ch = take ? r.y : rootward ? rr.z : dead ? 0u : st.opos_ch;
        st.fail = take ? r.z : rootward ? (rr.z & 0xffu) : dead ? 0u : st.fail;
        st.fmap = take ? r.w : rootward ? rr.w : dead ? 0u : st.fmap;
        return hit || dead || rootward;
    }

    // classic delta (failure links never stop): reference src/bytewise.rs:1063-1088 over fail_plain
    __device__ __forceinline__ void step_plain(RsState &st, uint32_t c) const {
        for (;;) {
            if (st.idx == 0) {
                const uint4 r = l_root[c];
                st = RsState{r.x, r.y, r.z};
                return;
            }
            if (st.base != 0) {
                const uint32_t child = st.base ^ c;
                const uint2 h = d.hot[child];
                if ((h.y & 0xffu) == c) { st = RsState{child, h.x, h.y}; return; }
            }
            const uint32_t f = d.fail_plain[st.idx];
            if (f == 0) { st.idx = 0; continue; }
            const uint2 h = d.hot[f];
            st = RsState{f, h.x, h.y};
        }
    }

    // next_state_id_leftmost_unchecked, reference src/bytewise.rs:1094-1128 (returns ROOT on DEAD)
    __device__ __forceinline__ void step_leftmost(RsState &st, uint32_t c) const {
        for (;;) {
            if (st.idx == 0) {  // at ROOT: the child if there is one, else stay (":1113-1116")
                const uint4 r = l_root[c];
                st = RsState{r.x, r.y, r.z};
                return;
            }
            if (st.base != 0) {
                const uint32_t child = st.base ^ c;
                const uint2 h = d.hot[child];
                if ((h.y & 0xffu) == c) { st = RsState{child, h.x, h.y}; return; }
            }
            const uint32_t f = d.fail[st.idx];
            if (f <= 1u) {  // DEAD (1): stop; ROOT (0): retry from the root row
                if (f == 1u) { st = RsState{0, 0, 0}; return; }
                st.idx = 0;
                continue;
            }
            const uint2 h = d.hot[f];
            st = RsState{f, h.x, h.y};
        }
    }

    // first sync point >= x: warm the classic automaton up over the halo, then run it to ROOT
    __device__ __forceinline__ uint64_t sync_from(const uint8_t *hay, uint64_t x, uint32_t halo, uint64_t floor, uint64_t len) const {
        if (x <= floor) return floor;  // the window start is a sync point by contract
        if (x >= len) return len;
        uint64_t pos = x > halo ? x - halo : 0;
        if (pos < floor) pos = floor;
        RsState st{0, 0, 0};
        while (pos < x) step_plain(st, hay[pos++]);
        while (st.idx != 0 && pos < len) step_plain(st, hay[pos++]);
        return st.idx == 0 ? pos : len;
    }
};

}  // namespace daac
