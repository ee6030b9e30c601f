// GRAM engine, `.count()` kernel of rounds 5-6 (gfx950): find_overlapping_iter(haystack).count() of a Standard bytewise automaton
// (reference loop: src/bytewise/iter.rs:133-176 over src/bytewise.rs:1063-1088) with ONE LDS lookup per haystack byte in the main
// path and six per hit.  Tables: gram4.hpp (M words, per-word rank directory, hit and walk records, "no pattern" as the last
// class).  Method: gram_kernels.hip / gram3_kernels.hip — no state chain; an occurrence of at most K bytes is a function of the
// last K classes (two count bits of the M word), a longer one is found from its start: continuation bit of its (K+1)-gram, the
// bit's rank, one record from L2, and a queued goto-only walk for the few branches that go on.
//
// What changed against gram3_kernels.hip and why (profiles/r04_pmc_sq.txt: 21.5 VALU and 3.85 wave-wide LDS accesses per
// haystack byte — at the rates of tools/micro/pipes_bench.hip both pipes were full at 1.3 TB/s):
//   * byte classes by arithmetic where the dictionary's bytes are one range (cfg3: a-z): class = min(byte - lo, C - 1), two
//     VALU and no LDS access — one lookup per byte less in the main path, six per hit less in the consumer;
//   * the rank of a hit from the PER-WORD directory (two LDS reads and one popcount instead of five reads and four): the
//     directory fits beside M once the class table is gone and a step is 16 positions per lane;
//   * the consumer builds one context index and scales it twice (M word, directory entry) instead of carrying an LDS address
//     through three multiply-adds, keeps the four text bytes behind a hit as they are (their classes are only worked out
//     for a record that can go on) and leaves the first child of a branch that goes on to the drain, which runs 64 such
//     branches wide where the batch that found them had three or four;
//   * hit records carry "ends a pattern" in bit 30 and no class needs the `!= 0` test in front of its child bit.
// Round 6: (a) a filter in front of rank + gather (gram4_filter.hpp; the FILT body below): 83 % of uniform text's hits neither end a
// pattern nor go on — a batch of hits is probed in one Bloom word per (K+1)-gram, what passes is re-compacted by a forward permute and
// ranked / gathered 64 at a time; the Bloom array lies where the per-word directory would, so workgroups whose text is made of
// dictionary words (their own probe) keep that directory and the TAIL body.  1 400 -> 1 500 GB/s on cfg3 (profiles/r06_gram4_decomposition.txt).
// (b) the hit queues hold 16-bit offsets into the wave's text slot (4 KB more for the Bloom array).  (c) walker positions are offsets
// from a 2 GiB epoch base: they no longer wrap when a walker crosses a multiple of 4 GiB.
// Round 7: the hit queue by a wave prefix sum — each lane's hits go to [its first index, + popc(H)) of a linear 256-entry list per wave, 5 VALU
// a turn instead of 9 (ballot, two mbcnt and a ring address every turn), batches of 64 cut once the step's hits are in; a step with more
// hits than the list holds runs the scan again on the rest.  The lists take 4 KB more than the rings did, out of the Bloom array.  cfg3
// 2.815 -> 2.746 ms per 4 GiB, word soup -5 %, 22.07 -> 21.38 VALU per byte (profiles/r07_gram4_decomposition.txt, r07_gram4_pmc_sq.txt).
// Round 8: fewer instructions per hit on the FILT path (profiles/r08_gram4_*.txt): the probe's word index is one v_mul_hi_u32_u24 and the
// ENDS rotation reads h's low bits as they are (gram4_filter.hpp); survivors that fail the probe all permute to one spare lane; rank_and_ask
// takes an ARITH hit's classes as byte - lo (a hit's bytes are pattern bytes: no min) and masks the group's words with one v_bfe_i32 each.
// Dropped: `derive` by two unaligned ds_read_b32 (five VALU fewer a batch, but an unaligned read is 7x slower than the aligned ones,
// tools/micro/lds_unaligned.hip).  Not done: survivors carrying a packed context index (the class work would move to every hit, 3.65 batches
// a step, from 1.6 survivor batches) and a finer coarse directory (its LDS comes out of the Bloom array).
// Round 9: the text fetch of an interior step — the whole step inside its region, none of its bytes among the haystack's first 16 or past its
// end, decided from the step's 32-bit offset in the region on the scalar unit — is Q loads at scalar base + the lane's offset + 16 q: no per-lane
// 64-bit position, no fill, no vlen / lead compares (30 VALU a step -> 1).  The first step of a scan and the fetches that reach past a region's or the
// haystack's end keep load_chunk.  The step loop counts that offset (32-bit) instead of a 64-bit position.  SQ_INSTS_VALU 20.06 -> 19.22 per byte
// and lane; cfg3 2.637 -> 2.594 ms per 4 GiB, cfg2 1.272 -> 1.159 ms (profiles/r09_gram4_*.txt): the instructions that went were cheaper than the rest.
// Round 10: a survivor of the filter finds its record by a perfect hash of its K+1 raw bytes (gram4_mph.hpp; MPH below) instead of by its rank: the
// displacement table (one byte a bucket) lies in LDS where the coarse directory lay, the records in slot order in dhit_h.  10 VALU and one ds_read_u8
// a batch of 64 survivors instead of 23 and four LDS reads; the TAIL body, the plain body and the density probe keep ranks.  A handle whose dictionary
// is too dense for a table that small keeps the rank path (build_gram4_mph says no).  profiles/r10_gram4_*.txt.
// Round 11: (a) a slab entry of the plain and FILT bodies is {record x, record y, position, text}: the gathered pair is stored from the registers
// it was loaded into — with the position first the compiler moved it one register up right behind the gather, and waited for it there.  (b) K = 3:
// the M-word address of an odd position from the even position's intermediate (gram4_index.hpp): five instructions a pair, not six.  (c) hit-list
// entries are LDS addresses of byte p - 3 (`derive` adds no base and subtracts no 3).  (d) the count sum is v_and_b32 and two v_bcnt_u32_b32 onto the
// region's count.  (e) the probe's pass mask is the two compares' masks or-ed on the scalar unit.  SQ_INSTS_VALU 18.51 -> 17.36 per byte and lane
// (profiles/r11_gram4_*.txt).
// Round 14: outside the step loop (profiles/r14_gram4_edges.txt: the waves of a launch ended 500 us apart).  The haystack's end is cut into small
// regions (gram4_claims.hpp); a wave's first regions are static — whole rounds of the launch's waves —, the rest it claims from a counter in the
// call's scratch; the launch's last workgroup stores the result, so one clear serves counter and count; the TAIL body asks for a region's first
// text where the region before it ends; g4_copy keeps four loads in flight.  cfg3 2.375 -> 2.323 ms per 4 GiB.
// Roofline: HBM bytes of haystack (1 B read per byte); integer/bit work only, no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <utility>

#include "device_tables.hpp"
#include "gram4_claims.hpp"
#include "gram4_filter.hpp"
#include "gram4_index.hpp"

namespace daac {

namespace {

typedef uint32_t g4_u32x4_t __attribute__((ext_vector_type(4)));
// batches of a pass of the FILT body at 32 / 16 positions per lane (round 13).  A pass keeps position, key bytes and text of each of its batches
// in registers: at 16 positions per lane that would cost the 64 VGPRs and with them the second workgroup of a CU, so those instances keep one
constexpr int kPass4Q2 = 2, kPass4Q1 = 1;
constexpr uint32_t kProbePercent4 = 3;  // density probe: TAIL when more than 3 % of the sampled positions start a walker
typedef __attribute__((address_space(3))) const uint32_t lds4_cu32;
typedef __attribute__((address_space(3))) uint32_t lds4_u32;
typedef __attribute__((address_space(3))) const uint16_t lds4_cu16;
typedef __attribute__((address_space(3))) uint16_t lds4_u16;
typedef __attribute__((address_space(3))) const uint8_t lds4_cu8;
typedef __attribute__((address_space(3))) g4_u32x4_t lds4_u32x4;

__device__ __forceinline__ uint32_t pin4(uint32_t x) {
    asm("" : "+v"(x));
    return x;
}
// a * b + c on the 24-bit multiplier (left to itself the compiler takes v_mad_u64_u32 here: a register pair, a move and an s_nop each)
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(b), "v"(c));
    return d;
}
// lane i <- lane i - 1 of `v`; lane 0 keeps `lane0`
__device__ __forceinline__ uint32_t wave_shr1_4(uint32_t v, uint32_t lane0) {
    uint32_t d = lane0;
    asm volatile("s_nop 1\nv_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(v));
    return d;
}
// inclusive sum over lanes 0 .. lane: four row shifts, two row broadcasts (a lane whose source is outside its row or whose row is
// masked off adds the 0 it was given as `old`)
__device__ __forceinline__ uint32_t g4_wave_scan(uint32_t v) {
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x111, 0xf, 0xf, false));   // row_shr:1
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x112, 0xf, 0xf, false));   // row_shr:2
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x114, 0xf, 0xf, false));   // row_shr:4
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x118, 0xf, 0xf, false));   // row_shr:8
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x142, 0xa, 0xf, false));   // row_bcast:15 (rows 1, 3)
    v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x143, 0xc, 0xf, false));   // row_bcast:31 (rows 2, 3)
    return v;
}
// f(integral_constant<int, 0>), f(.. 1>), .. while f returns true: a loop unrolled by hand (the compiler keeps a loop with a ballot in its
// exit test rolled)
template <typename F, int... I>
__device__ __forceinline__ void g4_turns(F &&f, std::integer_sequence<int, I...>) {
    (void)(... && f(std::integral_constant<int, I>{}));
}
// f(integral_constant<int, min(n, N)>) for a wave-uniform n >= 1
template <int N, typename F>
__device__ __forceinline__ void g4_upto(uint32_t n, F &&f) {
    if constexpr (N > 1) {
        if (n < static_cast<uint32_t>(N)) {
            g4_upto<N - 1>(n, f);
            return;
        }
    }
    f(std::integral_constant<int, N>{});
}
__device__ __forceinline__ unsigned long long g4_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ void g4_copy(void *dst, const void *src, uint32_t bytes) {
    const uint4 *s = reinterpret_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint32_t n = bytes / 16, bd = blockDim.x;
    uint32_t i = threadIdx.x;
    for (; i + 3u * bd < n; i += 4u * bd) {   // four loads of a thread in flight before its first LDS store (M: one round trip, not five)
        const uint4 v0 = s[i], v1 = s[i + bd], v2 = s[i + 2u * bd], v3 = s[i + 3u * bd];
        d[i] = v0; d[i + bd] = v1; d[i + 2u * bd] = v2; d[i + 3u * bd] = v3;
    }
    for (; i < n; i += bd) d[i] = s[i];
}
// The launch's count goes through the call's own block `claim` = {claims, count, workgroups done}, zero at launch (one clear for the claim
// counter and the count): every workgroup adds its count to claim[1], and the one that finishes last STORES the sum and two zeros to
// `result` — the caller's three words need no clear of their own in front of the launch.
__device__ __forceinline__ void g4_reduce(unsigned long long cnt, unsigned long long *scratch, unsigned long long *claim, unsigned long long *result) {
    const unsigned long long c = g4_wave_sum(cnt);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) scratch[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r0 = 0;
        for (int w = 0; w < static_cast<int>((blockDim.x + 63) >> 6); ++w) r0 += scratch[w];
        if (r0) atomicAdd(claim + 1, r0);
        __threadfence();   // the count is added before this workgroup counts as done
        if (atomicAdd(claim + 2, 1ull) + 1ull == gridDim.x) {
            __threadfence();
            result[0] = atomicAdd(claim + 1, 0ull);
            result[1] = 0;
            result[2] = 0;
        }
    }
}
// 16 bytes of text at virtual position v (a multiple of 16): what lies before the haystack's first byte or past its end reads as the unused byte
__device__ __forceinline__ uint4 g4_load_chunk(const GramArgs &a, uint32_t unused_byte, uint64_t v) {
    const uint32_t ub4 = unused_byte * 0x01010101u;
    if (v >= a.vlen) return uint4{ub4, ub4, ub4, ub4};
    const g4_u32x4_t q = __builtin_nontemporal_load(reinterpret_cast<const g4_u32x4_t *>(a.hay_al + v));
    uint4 r{q.x, q.y, q.z, q.w};
    if (v < a.lead || v + 16 > a.vlen) {  // first / last chunk of the haystack only
        uint32_t w[4] = {r.x, r.y, r.z, r.w};
        for (int b = 0; b < 16; ++b) {
            const uint64_t p = v + b;
            if (p < a.lead || p >= a.vlen) w[b >> 2] = (w[b >> 2] & ~(0xffu << (8 * (b & 3)))) | (unused_byte << (8 * (b & 3)));
        }
        r = uint4{w[0], w[1], w[2], w[3]};
    }
    return r;
}
// The text of the step at rbase + off of a region of rlen bytes, for the two fetches a region begins with (off = 0 and one step) where they
// are asked for ahead of the region (gram4_body's AHEAD).  Same values as gram4_body's `fetch` (its interior form where that applies:
// unconditional loads that nothing has to wait for here).
template <int Q>
__device__ __forceinline__ void g4_fetch_ahead(const GramArgs &a, uint32_t unused_byte, uint64_t rbase, uint32_t rlen, uint32_t off, uint4 (&out)[Q]) {
    constexpr uint32_t P = 16u * Q, SB = 64u * P;
    const uint32_t lane = threadIdx.x & 63, ub4 = unused_byte * 0x01010101u;
    const uint32_t fast_lo = rbase < 16u ? SB : 0u, fast_hi = rlen & ~(SB - 1u);
    if (off >= fast_lo && off < fast_hi) {
        const uint8_t *__restrict__ base = a.hay_al + rbase + off;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const g4_u32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const g4_u32x4_t *>(base + lane * P + 16u * q));
            out[q] = uint4{t.x, t.y, t.z, t.w};
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) out[q] = uint4{ub4, ub4, ub4, ub4};
    if (off < rlen) {
#pragma unroll
        for (int q = 0; q < Q; ++q) out[q] = g4_load_chunk(a, unused_byte, rbase + off + lane * P + 16u * q);
    } else if (lane == 0 && off < rlen + SB) {
        out[0] = g4_load_chunk(a, unused_byte, rbase + off);
    }
}

}  // namespace

// K = context length; Q = 16-byte chunks a lane takes per step (P = 16 Q positions); ARITH = classes by min(byte - lo, C - 1) (else the
// 256-byte table in LDS); DIR = 0: one u16 directory entry per M word, 1 / 2: one u16 / u32 entry per four words; TAIL = tail records
// from the hit record on and a second pending stage (text made of dictionary words); FILT = a batch of hits goes through the LDS
// filter of gram4_filter.hpp first and only what passes — collected 64 at a time — is ranked and asks the L2 for its record (round 6;
// coarse directory, plain records: text made of dictionary words passes the filter anyway and keeps the TAIL body)
// MPH (FILT only): a survivor's record by the perfect hash of gram4_mph.hpp on its K+1 raw bytes — dhit_h[slot] — instead of dhit_c[rank]; the
// displacement table lies where the coarse directory would (round 10)
template <int K, int Q, bool ARITH, int DIR, bool TAIL, bool FILT, bool MPH = false>
__device__ __forceinline__ void gram4_body(const Gram4Dev &g, const GramArgs &a, const Gram4Lds &L, char *smem) {
    static_assert(!(FILT && TAIL), "the filter runs in front of the plain records");
    static_assert(!(FILT && DIR == 0), "the filter's Bloom array lies where the per-word directory would");
    static_assert(!MPH || FILT, "the perfect hash serves the survivors of the filter");
    constexpr int P = 16 * Q;
    constexpr int GS = 8;
    constexpr int PB = !FILT ? 1 : Q == 2 ? kPass4Q2 : kPass4Q1;   // FILT: batches of 64 hits that go through the filter in lock-step (process_pass)
    constexpr uint32_t SB = 64u * P;          // bytes a wave takes per step
    constexpr uint32_t SLOT = SB + 32u;       // [12,16) the four bytes before the step | [16, 16 + SB) the step | 16 bytes of the next
    // ONE text slot per wave: what is left in the hit queue at the end of a step (fewer than 64 entries) has its text taken out of the
    // slot into registers before the next step's text goes in (`derive` below).  Two slots would not leave the per-word rank directory
    // room beside M at 32 positions per lane (cfg3: 79 + 39 KB of tables, 16 x 2.6 KB of slots and queues).
    const uint32_t offM = L.off_m, offS = L.off_s, offC = L.off_cls;
    const uint32_t lo = g.lo, OTH = g.C - 1u, C = g.C;
    auto cls_of = [&](uint32_t byte) -> uint32_t {
        if (ARITH) {
            const uint32_t u = byte - lo;
            return u < OTH ? u : OTH;
        }
        return *reinterpret_cast<lds4_cu8 *>(static_cast<uintptr_t>(offC + byte));
    };
    auto lds_u32 = [&](uint32_t addr) -> uint32_t { return *reinterpret_cast<lds4_cu32 *>(static_cast<uintptr_t>(addr)); };
    auto below = [&](uint32_t k) -> uint32_t { return (1u << k) - 1u; };  // k <= 29

    const uint32_t lane = threadIdx.x & 63;
    const uint32_t lane_off = pin4(lane * (16u * Q));   // this lane's share of a step, from the step's first byte (pinned: it stays a 32-bit
                                                        // offset beside a scalar base in the load, not a 64-bit add per chunk)
    const uint32_t wave_in_wg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t C4 = C * 4u, CC4 = C * C * 4u;
    const uint32_t offM1 = g4i_off1(offM, C);   // the second constant of an odd position's M-word address (gram4_index.hpp)
    const uint32_t ub4 = g.unused_byte * 0x01010101u;
    const uint8_t *__restrict__ hay = a.hay_al;
    const uint64_t nwaves = static_cast<uint64_t>(gridDim.x) * (blockDim.x >> 6);
    // per-wave LDS: the text slot; the hit lists of all waves come first
    const uint32_t tb = L.off_wave + wave_in_wg * L.wave_stride;   // wave-uniform
    const uint32_t listb = wave_in_wg * (kList4 * 2u);
    // this wave's slab of pending walkers, 16-byte entries.  plain: {hit record x, hit record y, position of the hit byte, the four text
    // bytes behind the hit} — the gathered pair first: it is stored from the registers it was loaded into, so nothing has to wait for it
    // where it was asked for (round 11) —; TAIL and what the drain writes back: {position, state | class << 27, text bytes from
    // position + 2 on, three more | how many << 24}
    const uint64_t slab_index = (static_cast<uint64_t>(blockIdx.x) * (blockDim.x >> 6) + wave_in_wg) * a.wq_slab;
    uint4 *__restrict__ slab4 = reinterpret_cast<uint4 *>(a.wq) + slab_index;
    // Positions in the queues, the pending stages and the slab are 32-bit offsets from `epoch_base`, a multiple of 2 GiB: a region (a power
    // of two of at most 1 GiB) lies inside one epoch, an offset stays below 2^31 + the longest pattern however far a walker moves on, and
    // the slab is emptied before the epoch changes.  (Until round 6 the epoch was 4 GiB and the offset the position's low word: a walker
    // that walked across a multiple of 4 GiB wrapped to 0 and read its text 4 GiB too early.)
    uint32_t wq_n = 0, slab_hi = 0;  // wave-uniform; slab_hi = epoch_base >> 31
    uint64_t epoch_base = 0;
    const uint32_t drain_early = wave_in_wg * 64u;   // the waves of a workgroup drain at different fill levels (they fill at the same pace: all
                                                     // sixteen waiting on the same round trips at once left the CU idle)

    unsigned long long tot_cnt = 0;
    uint32_t cnt32 = 0;  // matches of the current region (a region is far too short to overflow 32 bits)

    auto load_chunk = [&](uint64_t v) -> uint4 { return g4_load_chunk(a, g.unused_byte, v); };
    auto raw_at = [&](uint64_t p) -> uint32_t { return (p >= a.lead && p < a.vlen) ? hay[p] : g.unused_byte; };
    auto read_ahead = [&](uint64_t v) -> unsigned long long {
        unsigned long long x;
        if (v >= a.lead && v + 8 <= a.vlen) {
            __builtin_memcpy(&x, hay + v, 8);
        } else {
            x = 0;
            for (int b = 7; b >= 0; --b) x = (x << 8) | ((v + b >= a.lead && v + b < a.vlen) ? hay[v + b] : g.unused_byte);
        }
        return x;
    };
    // the rest of a subtree that is one path {1 << 31 | edges | word ends << 4, -, path bytes 0-3, path bytes 4-7} against the text
    auto tail_count = [&](const uint4 &rr, unsigned long long text) -> uint32_t {
        const uint32_t edges = rr.x & 15u;
        const unsigned long long path = (static_cast<unsigned long long>(rr.w) << 32) | rr.z;
        const unsigned long long diff = path ^ text;
        uint32_t same = diff ? static_cast<uint32_t>(__builtin_ctzll(diff)) >> 3 : 8u;
        same = same < edges ? same : edges;
        return __popc((rr.x >> 4) & ((2u << same) - 1u) & 0x1ffu);
    };
    // Finishes the queued branches.  One pass moves every branch ONE state on, 64 branches wide, and writes those that still go on
    // back to the front of the slab (compacted by ballot); passes repeat until nothing is left.  (Round 4's drain followed every
    // branch to its end inside one loop: the wave then runs as long as its deepest branch — on random text nine branches in ten end
    // at their first record, and the few that do not kept 64 lanes busy for five or six more rounds: 12 % of the kernel.)
    auto drain = [&]() {
        const uint4 *__restrict__ recs = TAIL ? g.drec_t : g.drec_c;
        uint32_t n_in = wq_n;
        bool raw = !TAIL;   // plain: the first pass reads what the batches left: {hit record x, hit record y, position, four text bytes}
        while (n_in != 0) {
            uint32_t n_out = 0;
            for (uint32_t base = 0; base < n_in; base += 64u) {
                const uint32_t i = base + lane;
                const bool live = i < n_in;
                uint4 e = uint4{0u, 0u, 0u, 0u};
                if (live) e = slab4[i];
                uint32_t state, n_ahead, pos = e.x;
                unsigned long long ah;
                if (raw) {
                    const uint32_t k1 = cls_of(e.w & 0xffu);
                    state = e.y + __popc(e.x & below(k1));
                    pos = e.z;
                    ah = e.w >> 8;
                    n_ahead = 3;
                } else {
                    state = e.y & 0x07ffffffu;
                    ah = (static_cast<unsigned long long>(e.w & 0xffffffu) << 32) | e.z;  // the bytes from vnext on (e.w >> 24 of them)
                    n_ahead = e.w >> 24;
                }
                uint4 rr = uint4{0u, 0u, 0u, 0u};
                if (live) rr = recs[state];  // {cmap, first_child, own_cnt, -} or a tail record
                const uint64_t vn = epoch_base + pos + 2;  // the state consumed the byte before vn
                bool cont = false;
                uint32_t next_state = 0;
                if (rr.x >> 31) {   // the rest is one path (idle lanes: a zero record, nothing happens)
                    if (n_ahead < (rr.x & 15u)) ah = read_ahead(vn);
                    cnt32 += tail_count(rr, ah);
                } else {
                    if (live && n_ahead == 0u) { ah = read_ahead(vn); n_ahead = 8; }
                    const uint32_t k = cls_of(static_cast<uint32_t>(ah) & 0xffu);
                    cnt32 += rr.z;
                    cont = ((rr.x >> k) & 1u) != 0;   // (the class of no pattern has no bit in a child map)
                    next_state = rr.y + __popc(rr.x & below(k));
                }
                const unsigned long long m = __ballot(cont);
                if (m != 0) {
                    if (cont) {
                        const uint32_t at = n_out + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0));
                        ah >>= 8;
                        slab4[at] = uint4{pos + 1u, next_state, static_cast<uint32_t>(ah), static_cast<uint32_t>(ah >> 32) | ((n_ahead - 1u) << 24)};
                    }
                    n_out += static_cast<uint32_t>(__popcll(m));
                }
            }
            n_in = n_out;
            raw = false;
        }
        wq_n = 0;
    };

    // ---- the hit list: entry = LDS address of byte p - 3 of the hit byte p in the wave's text slot (u16: the lists and slots end below 64 KB;
    // round 11 — an offset from the slot's start cost `derive` an add of the slot's base and a subtract of 3 in every batch)
    uint32_t q_head = 0, q_tail = 0;   // wave-uniform: entries [q_head, q_tail) of the list are queued, not yet taken
    uint32_t posbias = 0;              // (virtual position of a hit byte - epoch_base) - (its list entry), of the text in the slot
    uint32_t st_n = 0;                 // wave-uniform: lanes [0, st_n) hold an entry of the NEXT batch already taken out of queue and slot
    uint32_t pend_lo = 0;              // the bytes p-3 .. p of the next batch's entry (p = its hit byte); pend_pos / pend_t0 / pend_t1 go with it
    uint4 pend = uint4{0u, 0u, 0u, 0u};  // record read for the previous batch, not yet consumed; zero for idle lanes
                                         // {cmap | ends-a-pattern << 30, first_child, -, -}; TAIL: or a tail record
    uint32_t pend_pos = 0;             // position of the hit byte
    uint32_t pend_t0 = 0, pend_t1 = 0; // the four bytes from position + 1 on; TAIL: and the four behind them
    bool pend_valid = false;           // wave-uniform
    // TAIL: a branch that goes on past the hit's state asks for the record of the NEXT state at once (p2, looked at one batch later)
    uint4 p2 = uint4{0u, 0u, 0u, 0u};    // record of the state below the hit's; zero for idle lanes
    uint32_t p2_pos = 0, p2_state = 0;   // position of the hit byte; the state asked for | class of the byte at position + 2 << 27
    uint32_t p2_t0 = 0, p2_t1 = 0;       // the seven bytes from position + 2 on
    bool p2_live = false, p2_any = false;        // per lane / wave-uniform
    // FILT: what has passed the filter waits in lanes [0, sb_n) — position, the four bytes up to the hit byte, the four behind it — until 64
    // are together; the batch whose records are in flight then has its position and text in fp_pos / fp_t0 (pend_* belong to the batch
    // that is going through the filter)
    uint32_t sb_n = 0;                 // wave-uniform
    uint32_t sb_pos = 0, sb_lo = 0, sb_t0 = 0;
    uint32_t fp_pos = 0, fp_t0 = 0;
    const uint32_t offB = L.off_b, bloomW = g.bloom_words;
    auto push_walker = [&](bool go, const uint4 &entry) {
        const unsigned long long m = __ballot(go);
        if (m != 0) {
            if (go) {
                const uint32_t at = wq_n + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0));
                slab4[at] = entry;
            }
            wq_n += __popcll(m);
        }
    };
    auto finish_second = [&]() {
        if (!TAIL || !p2_any) return;
        p2_any = false;
        const uint4 r = p2;
        bool again = false;           // still going on: to the slab (or a tail of eight edges: the drain has the eighth byte fetched)
        uint32_t st_k = 0, pos = p2_pos, t0 = p2_t0, t1n = (p2_t1 & 0xffffffu) | (7u << 24);
        if (p2_live) {
            if (r.x >> 31) {
                if ((r.x & 15u) <= 7u) cnt32 += tail_count(r, (static_cast<unsigned long long>(p2_t1) << 32) | p2_t0);
                else { again = true; st_k = p2_state; }  // eight edges, seven bytes at hand: the drain looks at the record again with the eighth byte fetched
            } else {
                cnt32 += r.z;
                const uint32_t k = p2_state >> 27;
                if ((r.x >> k) & 1u) {
                    again = true;
                    const uint32_t k3 = cls_of((p2_t0 >> 8) & 0xffu);
                    st_k = (r.y + __popc(r.x & below(k))) | (k3 << 27);
                    pos = p2_pos + 1u;
                    t0 = __builtin_amdgcn_alignbyte(p2_t1, p2_t0, 1u);
                    t1n = ((p2_t1 >> 8) & 0xffffu) | (6u << 24);
                }
            }
        }
        p2_live = false;
        push_walker(again, uint4{pos, st_k, t0, t1n});
    };
    auto consume_pending = [&]() {
        finish_second();
        if (!pend_valid) return;
        pend_valid = false;
        const uint4 r = pend;
        if (FILT) {
            const uint32_t k1 = cls_of(fp_t0 & 0xffu);
            cnt32 += (r.x >> kGram4EndsBitDev) & 1u;
            push_walker(__builtin_amdgcn_ubfe(r.x, k1, 1) != 0, uint4{r.x, r.y, fp_pos, fp_t0});
            return;
        }
        const uint32_t k1 = cls_of(pend_t0 & 0xffu);
        if (!TAIL) {
            cnt32 += (r.x >> kGram4EndsBitDev) & 1u;
            // (the first child of a branch that goes on is worked out in the drain, 64 branches wide: here three or four lanes of 64 go on)
            push_walker(__builtin_amdgcn_ubfe(r.x, k1, 1) != 0, uint4{r.x, r.y, pend_pos, pend_t0});
            return;
        }
        bool go;
        if (r.x >> 31) {  // one path below the hit: settled here
            cnt32 += tail_count(r, (static_cast<unsigned long long>(pend_t1) << 32) | pend_t0);
            go = false;
        } else {
            cnt32 += (r.x >> kGram4EndsBitDev) & 1u;
            go = ((r.x >> k1) & 1u) != 0;
        }
        p2 = uint4{0u, 0u, 0u, 0u};
        p2_live = go;
        p2_any = __ballot(go) != 0;
        if (go) {
            const uint32_t child = r.y + __popc(r.x & below(k1));
            const uint32_t k2 = cls_of((pend_t0 >> 8) & 0xffu);
            p2 = g.drec_t[child];
            p2_pos = pend_pos;
            p2_state = child | (k2 << 27);
            p2_t0 = __builtin_amdgcn_alignbyte(pend_t1, pend_t0, 1u);  // text from position + 2 on
            p2_t1 = pend_t1 >> 8;
        }
    };
    // Takes `cnt` entries from the head of the list into lanes [first, first + cnt): position, the four bytes up to the hit byte, the
    // four (TAIL: eight) behind it.  After this the entries no longer refer to the slot.
    auto derive = [&](uint32_t first, uint32_t cnt) {
        if (lane - first < cnt) {
            const uint32_t t3 = *reinterpret_cast<lds4_cu16 *>(static_cast<uintptr_t>(listb + ((q_head + lane - first) << 1)));
            pend_pos = t3 + posbias;
            const uint32_t a0 = t3 & ~3u, sh = t3 & 3u;
            // the dwords around the hit byte (the slot is self-contained: never outside [slot + 12, slot + SLOT)).  (Round 8 tried two
            // ds_read_b32 at the byte address instead: 7x slower than these reads on gfx950, tools/micro/lds_unaligned.hip)
            const uint32_t d0 = lds_u32(a0), d1 = lds_u32(a0 + 4u), d2 = lds_u32(a0 + 8u);
            pend_lo = __builtin_amdgcn_alignbyte(d1, d0, sh);              // bytes p-3 .. p
            pend_t0 = __builtin_amdgcn_alignbyte(d2, d1, sh);              // bytes p+1 .. p+4
            if (TAIL) {
                const uint32_t d3 = lds_u32(a0 + 12u);
                pend_t1 = __builtin_amdgcn_alignbyte(d3, d2, sh);          // bytes p+5 .. p+8
            }
        }
        q_head += cnt;
    };
    // rank of the hit whose bytes p-3 .. p are x_lo -> its record asked for (into `pend`)
    // (ARITH: the K+1 bytes of a hit are all pattern bytes, so their classes are byte - lo without the min — the context index is two
    // multiply-adds of selected bytes with the bias folded in, round 8)
    const uint32_t lo_idx = K == 3 ? lo * (C * C + C + 1u) : lo * (C + 1u);
    auto rank_and_ask = [&](uint32_t x_lo) {
        uint32_t idx, d;
        if (ARITH) {
            idx = mad24((x_lo >> 8) & 0xffu, C, ((x_lo >> 16) & 0xffu) - lo_idx);
            if (K == 3) idx = mad24(x_lo & 0xffu, C * C, idx);
            d = (x_lo >> 24) - lo;
        } else {
            const uint32_t c1 = cls_of((x_lo >> 8) & 0xffu), c2 = cls_of((x_lo >> 16) & 0xffu);
            d = cls_of(x_lo >> 24);
            idx = __umul24(c1, C) + c2;
            if (K == 3) idx = __umul24(cls_of(x_lo & 0xffu), C * C) + idx;
        }
        // rank of continuation bit d of that M word among all set bits = offset of the depth-(K+1) state
        const uint32_t am = (idx << 2) + offM;
        const uint32_t own = lds_u32(am);
        uint32_t rank;
        if (DIR == 0) {
            const uint32_t base = *reinterpret_cast<lds4_cu16 *>(static_cast<uintptr_t>((idx << 1) + offS));
            rank = base + __popc(own & below(d));
        } else {
            const uint32_t grp = am & ~15u;   // (M starts 16-byte aligned)
            const uint32_t qx = lds_u32(grp), qy = lds_u32(grp + 4u), qz = lds_u32(grp + 8u);
            const uint32_t gi = pin4(idx >> 2);   // (pinned: one v_lshl_add_u32 below, not a shift, a mask and an add)
            const uint32_t base = DIR == 1 ? *reinterpret_cast<lds4_cu16 *>(static_cast<uintptr_t>((gi << 1) + offS))
                                           : *reinterpret_cast<lds4_cu32 *>(static_cast<uintptr_t>((gi << 2) + offS));
            // word j of the group counts when it lies before the hit's, i.e. bit idx & 3 of 0b1110 / 0b1100 / 0b1000 is set: one v_bfe_i32
            // of the nibble repeated eight times, at offset idx (the instruction reads bits 4:0 of the offset) gives all ones or zero
            const uint32_t mx = static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(0xEEEEEEEEu), idx, 1u));
            const uint32_t my = static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(0xCCCCCCCCu), idx, 1u));
            const uint32_t mz = static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(0x88888888u), idx, 1u));
            uint32_t under = __popc(own & below(d));
            under += __popc(qx & mx & 0x3fffffffu);
            under += __popc(qy & my & 0x3fffffffu);
            under += __popc(qz & mz & 0x3fffffffu);
            rank = base + under;
        }
        if (TAIL) {
            pend = g.dhit_t[rank];
        } else {
            const uint2 h = g.dhit_c[rank];
            pend = uint4{h.x, h.y, 0u, 0u};
        }
    };
    // MPH: the record of the hit whose bytes p-3 .. p are x_lo asked for by the hash of its K+1 raw bytes — no class, no M word, no directory:
    // h and f (2 VALU each: the top byte's product by an SDWA byte select, one v_mad_u32_u24; h is worked out again here rather than carried
    // from the probe through a fourth ds_permute in every batch of hits, 3.65 a step against 1.6 of these), the bucket and its LDS address (2),
    // one ds_read_u8, the slot (3), the record's address (1): 10 VALU and 1 LDS read where rank_and_ask takes 23 and 4 (profiles/r10_gram4_isa.txt)
    const G4Mph mph = g.mph;
    auto hash_and_ask = [&](uint32_t x_lo) {
        const uint32_t x = K == 3 ? x_lo : x_lo >> 8;
        const uint32_t h = g4f_h(x);
        const uint32_t d = *reinterpret_cast<lds4_cu8 *>(static_cast<uintptr_t>(offS + g4m_bucket(h, mph)));
        const uint2 r = g.dhit_h[g4m_slot(h, g4m_f(x, mph), d, mph)];
        pend = uint4{r.x, r.y, 0u, 0u};
    };
    // FILT, second stage at the end of a scan: the n < 64 survivors still waiting in lanes [0, n) of sb_* are ranked (MPH: hashed) and ask for their
    // records (a full set of 64 is asked for where it comes together, in process_batch)
    auto survivors_ask = [&](uint32_t n) {
        consume_pending();
        pend = uint4{0u, 0u, 0u, 0u};
        if (lane < n) { if constexpr (MPH) hash_and_ask(sb_lo); else rank_and_ask(sb_lo); }
        // (taken by moves the compiler does not see through: as plain copies fp_* and sb_* shared a name on one path and were swapped where the paths
        // meet — round 12)
        uint32_t t0;
        asm("v_mov_b32_e32 %0, %1" : "=v"(fp_pos) : "v"(sb_pos));
        asm("v_mov_b32_e32 %0, %1" : "=v"(t0) : "v"(sb_t0));
        fp_t0 = lane < n ? t0 : 0u;   // (an idle lane: nothing of it may look like a branch that goes on)
        pend_valid = true;
    };
    auto process_batch = [&](uint32_t n) {  // n <= 64 entries: the st_n already taken out + the head of the queue
        __builtin_amdgcn_s_setprio(2);
        if (FILT) {
            derive(st_n, n - st_n);
            st_n = 0;
            // first stage: the probe of gram4_filter.hpp on the raw bytes p-K .. p and p + 1 — one word, the GO key's two bits or the ENDS key's four
            const G4Probe pr = g4f_probe(K == 3 ? pend_lo : pend_lo >> 8, pend_t0 & 0xffu, bloomW);
            const uint32_t fw = lds_u32(offB + (pr.word << 2));
            // (the two compares' masks or-ed and cut to the batch's lanes on the scalar unit: as one bool the compiler rebuilt the ballot
            // from a v_cndmask_b32 and a third compare — round 11)
            const unsigned long long in_batch = n >= 64u ? ~0ull : (1ull << n) - 1ull;
            const unsigned long long pm = (__builtin_amdgcn_ballot_w64((pr.go & ~fw) == 0u) | __builtin_amdgcn_ballot_w64((pr.ends & ~fw) == 0u)) & in_batch;
            if (pm != 0) {
                // survivors move to lanes sb_n, sb_n + 1, .. (mod 64) — one forward permute per word; the others all go to lane sb_n - 1 (mod 64),
                // which is outside [sb_n, sb_n + s) unless all 64 pass, and whose value is not looked at (round 8: before, they filled the lanes in
                // between, three VALU more) —
                const uint32_t s = static_cast<uint32_t>(__popcll(pm));
                const uint32_t r = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(pm >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(pm), 0));
                uint32_t t;   // rank among the survivors, 63 for the others (the ballot as the mask: left to itself the compiler branches on it)
                asm("v_cndmask_b32_e64 %0, 63, %1, %2" : "=v"(t) : "v"(r), "s"(pm));
                const uint32_t tgt = ((t + sb_n) << 2) & 0xfcu;
                const uint32_t r_pos = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(static_cast<int>(tgt), static_cast<int>(pend_pos)));
                const uint32_t r_lo = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(static_cast<int>(tgt), static_cast<int>(pend_lo)));
                const uint32_t r_t0 = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(static_cast<int>(tgt), static_cast<int>(pend_t0)));
                // lanes [sb_n, sb_n + s) below 64 join the waiting ones; what went beyond lane 63 arrived in lanes [0, sb_n + s - 64).  Both as
                // scalar masks, and every select written out on the register it keeps: sb_* stay where they are on both exits, nothing is renamed
                // where they meet (round 12: with `mine` a per-lane compare, the select into new names and the set assigned as a whole after the
                // 64 were asked for, the two exits met in ten and five v_mov_b32, 3.65 times a step)
                const bool full = sb_n + s >= 64u;
                unsigned long long mine;   // s < 64: the lanes [sb_n, sb_n + s) — one scalar instruction
                asm("s_bfm_b64 %0, %1, %2" : "=s"(mine) : "s"(s), "s"(sb_n));
                sb_n += s;
                if (full) {   // 64 together: the waiting ones below the old sb_n, the arrivals from there on — hashed (ranked) and asked for straight
                              // from the select, which leaves their position and text where the slab's store takes them from (the old ones consumed first)
                    consume_pending();
                    const unsigned long long upper = ~0ull << (sb_n - s);
                    uint32_t lo64;
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(fp_pos) : "v"(sb_pos), "v"(r_pos), "s"(upper));
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(lo64) : "v"(sb_lo), "v"(r_lo), "s"(upper));
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(fp_t0) : "v"(sb_t0), "v"(r_t0), "s"(upper));
                    if constexpr (MPH) hash_and_ask(lo64); else rank_and_ask(lo64);
                    pend_valid = true;
                    sb_n -= 64u;
                    asm("s_bfm_b64 %0, %1, 0" : "=s"(mine) : "s"(sb_n));   // the lanes that wrapped: [0, sb_n)
                }
                asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(sb_pos) : "v"(r_pos), "s"(mine));
                asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(sb_lo) : "v"(r_lo), "s"(mine));
                asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(sb_t0) : "v"(r_t0), "s"(mine));
            }
            return;
        }
        consume_pending();
        derive(st_n, n - st_n);
        st_n = 0;
        pend = uint4{0u, 0u, 0u, 0u};
        if (lane < n) {
            rank_and_ask(pend_lo);
        } else {
            pend_t0 = 0;   // (an idle lane: nothing of it may look like a branch that goes on)
            pend_t1 = 0;
        }
        pend_valid = true;
    };

    // FILT, round 13: the full batches a step has queued go through the filter in passes of up to PB, in lock-step: every stage of the chain —
    // list entry, text, Bloom word, permute, each an LDS round trip that the next stage's address waits for — is asked for in ALL the pass's
    // batches before the first answer is looked at, so a pass of NB batches waits four round trips, not 4 NB.  The body is compiled once per
    // NB = 1 .. PB, each straight code (a stage under a per-batch branch got its wait inside the branch, in front of the next batch's read).
    // Batch 0 takes the st_n entries already taken out plus the head of the list, the others are wholly from the list.  The ballots give every
    // batch's pass mask, its survivor count and with them the fill of the waiting set each batch will meet (all scalar) before any permute is
    // asked for; the joins then run in batch order exactly as process_batch's: a second set of 64 that comes together in one pass consumes
    // the first's records before it asks for its own.  The permutes are not skipped for a batch of which nothing passes (all its lanes then
    // target lane fill - 1; its join is skipped).  Measured forms that were slower than this one, some slower than one batch at a time
    // (profiles/r13_gram4_decomposition.txt): the joins as one copy behind the stages of every NB, the caller's loop kept from peeling
    // its first pass (`#pragma nounroll`), the permutes under `pm != 0`, and PB = 3 or 4.
    auto process_pass = [&](auto nbc) {
        constexpr int NB = decltype(nbc)::value;
        __builtin_amdgcn_s_setprio(2);
        // batch 0: lanes [0, st_n) hold their entry in pend_* already; they read the list's head entry like lane st_n (a queued entry: st_n < 64),
        // so every lane's reads stay inside list and slot and no stage of the batch sits under an exec mask
        const uint32_t i0 = static_cast<uint32_t>(std::max(static_cast<int>(lane - st_n), 0));
        const uint32_t la = listb + ((q_head + i0) << 1);                  // batch 0's list entry; batch b >= 1: lane's own, 64 b - st_n further on
        const uint32_t lb = listb + ((q_head + lane - st_n) << 1);
        uint32_t t3[NB], pos[NB], lo4[NB], t0[NB];
        // ---- all list reads ----
        t3[0] = *reinterpret_cast<lds4_cu16 *>(static_cast<uintptr_t>(la));
#pragma unroll
        for (int b = 1; b < NB; ++b) t3[b] = *reinterpret_cast<lds4_cu16 *>(static_cast<uintptr_t>(lb + 128u * b));
        q_head += 64u * NB - st_n;
        // ---- all text reads (the three dwords around the hit byte, as in `derive`), then the alignbytes ----
        uint32_t d0[NB], d1[NB], d2[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const uint32_t a0 = t3[b] & ~3u;
            d0[b] = lds_u32(a0); d1[b] = lds_u32(a0 + 4u); d2[b] = lds_u32(a0 + 8u);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            pos[b] = t3[b] + posbias;
            lo4[b] = __builtin_amdgcn_alignbyte(d1[b], d0[b], t3[b] & 3u);   // bytes p-3 .. p
            t0[b] = __builtin_amdgcn_alignbyte(d2[b], d1[b], t3[b] & 3u);    // bytes p+1 .. p+4
        }
        {   // (st_n != 0 only in the first pass after a step that left entries behind)
            const bool old = lane < st_n;
            pos[0] = old ? pend_pos : pos[0];
            lo4[0] = old ? pend_lo : lo4[0];
            t0[0] = old ? pend_t0 : t0[0];
            st_n = 0;
        }
        // ---- all probe hashes and Bloom word reads ----
        G4Probe pr[NB];
        uint32_t fw[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            pr[b] = g4f_probe(K == 3 ? lo4[b] : lo4[b] >> 8, t0[b] & 0xffu, bloomW);
            fw[b] = lds_u32(offB + (pr[b].word << 2));
        }
        // ---- all ballots: pass masks, survivor counts and the waiting set's fill in front of every batch, on the scalar unit ----
        unsigned long long pm[NB];
        uint32_t fill[NB];
        uint32_t cur = sb_n;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            pm[b] = __builtin_amdgcn_ballot_w64((pr[b].go & ~fw[b]) == 0u) | __builtin_amdgcn_ballot_w64((pr[b].ends & ~fw[b]) == 0u);
            fill[b] = cur;
            cur = (cur + static_cast<uint32_t>(__popcll(pm[b]))) & 63u;
        }
        // ---- all permute targets and permutes: survivors to lanes fill, fill + 1, .. (mod 64), the others to lane fill - 1 (process_batch) ----
        uint32_t r_pos[NB], r_lo[NB], r_t0[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const uint32_t r = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(pm[b] >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(pm[b]), 0));
            uint32_t t;
            asm("v_cndmask_b32_e64 %0, 63, %1, %2" : "=v"(t) : "v"(r), "s"(pm[b]));
            const uint32_t tgt = ((t + fill[b]) << 2) & 0xfcu;
            r_pos[b] = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(static_cast<int>(tgt), static_cast<int>(pos[b])));
            r_lo[b] = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(static_cast<int>(tgt), static_cast<int>(lo4[b])));
            r_t0[b] = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(static_cast<int>(tgt), static_cast<int>(t0[b])));
        }
        // ---- the joins, in batch order (sb_n is fill[b] when batch b's turn comes); the selects as process_batch pins them ----
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (pm[b] != 0) {
                const uint32_t s = static_cast<uint32_t>(__popcll(pm[b]));
                const bool full = sb_n + s >= 64u;
                unsigned long long mine;
                asm("s_bfm_b64 %0, %1, %2" : "=s"(mine) : "s"(s), "s"(sb_n));
                sb_n += s;
                if (full) {
                    consume_pending();
                    const unsigned long long upper = ~0ull << (sb_n - s);
                    uint32_t lo64;
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(fp_pos) : "v"(sb_pos), "v"(r_pos[b]), "s"(upper));
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(lo64) : "v"(sb_lo), "v"(r_lo[b]), "s"(upper));
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(fp_t0) : "v"(sb_t0), "v"(r_t0[b]), "s"(upper));
                    if constexpr (MPH) hash_and_ask(lo64); else rank_and_ask(lo64);
                    pend_valid = true;
                    sb_n -= 64u;
                    asm("s_bfm_b64 %0, %1, 0" : "=s"(mine) : "s"(sb_n));
                }
                asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(sb_pos) : "v"(r_pos[b]), "s"(mine));
                asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(sb_lo) : "v"(r_lo[b]), "s"(mine));
                asm("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(sb_t0) : "v"(r_t0[b]), "s"(mine));
            }
    };
    // the full batches queued so far: FILT with PB > 1 in passes of min(what is queued, PB), everything else one batch at a time
    auto process_full = [&]() {
        while (st_n + q_tail - q_head >= 64u) {
            if constexpr (FILT && PB > 1) g4_upto<PB>((st_n + q_tail - q_head) >> 6, process_pass);
            else process_batch(64u);
        }
    };

    // Regions are claimed, not owned (round 14).  A wave's first a.static_rounds regions are its own number in the launch plus multiples of
    // nwaves — no wave waits for an atomic before its first byte —; every further one is the next value of the call's counter
    // a.claim[0], which starts at 0 and stands for region static_rounds * nwaves: one relaxed agent-scope add by lane 0, broadcast to the
    // wave.  (The host makes every whole round of large regions static: all waves of a launch start within 2 us of each other, and 4 096
    // adds to one address at once queue for 60 us at the L2 — measured, profiles/r14_gram4_edges.txt; by the last static round the waves
    // are hundreds of microseconds apart.)  The claim for the region after this one goes out at this region's start, behind its first text
    // fetches, and comes back with them.  A claim index is turned into bytes by g4_claim_region: large regions first, small ones at the
    // haystack's end, where they even out the finish times of the waves.
    // INVARIANT the epoch logic below rests on: the regions of a wave ascend.  Its static indices ascend and lie below static_rounds * nwaves,
    // every claim is at least that, and the counter only grows, so a later claim of the same wave is larger than an earlier one; g4_claim_region is monotone in
    // the index.  A wave therefore never returns to an earlier 2 GiB epoch, and the slab is drained whenever the epoch changes.
    // (Region indices, their number and the claims fit 32 bits — every wave claims once more than it scans, and the host refuses a launch
    // whose regions + waves reach 2^32 —, so the low word of the 64-bit counter is the claim; the sizes go by their logarithms: fewer scalar registers live
    // through the step loop than 64-bit indices and sizes took.)
    const uint32_t nregions = static_cast<uint32_t>(a.nregions), nlarge = static_cast<uint32_t>(a.nlarge), nwaves32 = static_cast<uint32_t>(nwaves);
    const uint32_t lg_large = static_cast<uint32_t>(__builtin_ctzll(a.region_bytes)), lg_small = static_cast<uint32_t>(__builtin_ctzll(a.region_small));
    const uint32_t claim_base = nwaves32 * a.static_rounds;
    uint32_t static_left = a.static_rounds - 1u;   // static regions of this wave behind the current one
    auto claim_next = [&]() -> uint32_t {
        unsigned long long c = 0;
        if (lane == 0) c = __hip_atomic_fetch_add(a.claim, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return claim_base + __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(c));
    };
    auto region_of = [&](uint32_t r) -> G4Region { return g4_claim_region(r, lg_large, lg_small, nlarge); };
    uint32_t region = blockIdx.x * (blockDim.x >> 6) + wave_in_wg;
    // pf0 / pf1: the text of the next two steps, the step loop's own registers.  AHEAD (the TAIL body at 32 positions per lane): a region
    // finds its first two steps in them, asked for where the region before it ends (after the drain, if the epoch changes) and in front of
    // the region's own dependent loads (the bytes before it, their M word).  Measured (profiles/r14_gram4_edges.txt): word soup -4 %; the
    // FILT body +2 % on uniform text (102 VGPRs for 92), so it and the plain body ask at the region's start, as until round 14; at 16
    // positions per lane the text held across a region's end would cost the 64-VGPR budget that lets two workgroups share a CU.
    constexpr bool AHEAD = Q == 2 && TAIL;
    uint4 pf0[Q], pf1[Q];
    auto fetch_ahead = [&](uint32_t r) {
        const G4Region rg = region_of(r);
        const uint32_t len = static_cast<uint32_t>((rg.base + rg.size < a.vlen ? rg.base + rg.size : a.vlen) - rg.base);
        g4_fetch_ahead<Q>(a, g.unused_byte, rg.base, len, 0u, pf0);
        g4_fetch_ahead<Q>(a, g.unused_byte, rg.base, len, SB, pf1);
    };
    if constexpr (AHEAD) if (region < nregions) fetch_ahead(region);
    while (region < nregions) {
      slab_hi = static_cast<uint32_t>(region_of(region).base >> 31);
      epoch_base = static_cast<uint64_t>(slab_hi) << 31;
      for (;;) {
        const G4Region rg = region_of(region);
        const uint64_t rbase = rg.base;
        const uint64_t rend = rbase + rg.size < a.vlen ? rbase + rg.size : a.vlen;
        // classes of the K bytes before the region, oldest in the low byte; the four raw bytes before it
        uint32_t carry = 0, tail4 = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) carry |= (rbase >= static_cast<uint64_t>(K - i) ? cls_of(raw_at(rbase - (K - i))) : OTH) << (8 * i);
#pragma unroll
        for (int i = 0; i < 4; ++i) tail4 |= (rbase >= static_cast<uint64_t>(4 - i) ? raw_at(rbase - (4 - i)) : static_cast<uint32_t>(g.unused_byte)) << (8 * i);
        tail4 = __builtin_amdgcn_readfirstlane(tail4);
        carry = __builtin_amdgcn_readfirstlane(carry);
        uint32_t mcarry;  // M word of the K-gram ending just before the region
        {
            uint32_t x = (((carry >> (8 * (K - 1))) & 0xffu) << 2) + offM;
            x += __umul24((carry >> (8 * (K - 2))) & 0xffu, C4);
            if (K == 3) x += __umul24(carry & 0xffu, CC4);
            mcarry = __builtin_amdgcn_readfirstlane(lds_u32(x));
        }

        // The chunks of the step at rbase + off.  Where the step lies inside the region and no byte of it can be the haystack's first 16 or
        // lie past its end — decided on `off` alone, 32-bit and wave-uniform: a region is at most 1 GiB — the load is scalar base + the
        // lane's loop-invariant offset + 16 q as the immediate: no per-lane 64-bit position, no fill, no vlen / lead tests (round 9).  The
        // others — the first step of a scan, a step that reaches past the region's or the haystack's end — go through load_chunk as before;
        // past the region's end only lane 0's first chunk (it feeds the last step's trailer).
        const uint32_t rlen = static_cast<uint32_t>(rend - rbase);
        const uint32_t fast_lo = rbase < 16u ? SB : 0u;     // (lead < 16: only a chunk below 16 can begin before it)
        const uint32_t fast_hi = rlen & ~(SB - 1u);         // off < fast_hi: the whole step ends at or before rend <= vlen
        auto fetch = [&](uint32_t off, uint4 (&out)[Q]) {
            if (off >= fast_lo && off < fast_hi) {
                const uint8_t *__restrict__ base = hay + rbase + off;
                uint32_t voff = lane_off;
                asm volatile("" : "+v"(voff));   // (taken here: left to itself the compiler hoists hay + rbase + lane_off and adds `off` per lane, 64-bit)
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const g4_u32x4_t t = __builtin_nontemporal_load(reinterpret_cast<const g4_u32x4_t *>(base + voff + 16u * q));
                    out[q] = uint4{t.x, t.y, t.z, t.w};
                }
                return;
            }
            const uint64_t s0 = rbase + off;
#pragma unroll
            for (int q = 0; q < Q; ++q) out[q] = uint4{ub4, ub4, ub4, ub4};
            if (off < rlen) {
#pragma unroll
                for (int q = 0; q < Q; ++q) out[q] = load_chunk(s0 + lane * P + 16u * q);
            } else if (lane == 0 && off < rlen + SB) {
                out[0] = load_chunk(s0);
            }
        };
        if constexpr (!AHEAD) {
            fetch(0u, pf0);
            fetch(SB, pf1);
        }
        uint32_t region_next = region + nwaves32;
        if (static_left != 0) --static_left; else region_next = claim_next();
        const uint32_t rbias = static_cast<uint32_t>(rbase - epoch_base) - (tb + 16u - 3u);   // posbias of the region's first step (the entry of a hit byte lies 3 below its address)

        for (uint32_t off = 0; off < rlen; off += SB) {
            if (wq_n + 64u * P + 128u + drain_early > a.wq_slab) drain();
            uint4 cur[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) { cur[q] = pf0[q]; pf0[q] = pf1[q]; }
            consume_pending();  // before the next chunk is requested: loads retire in order
            __builtin_amdgcn_s_setprio(0);
            fetch(off + 2u * SB, pf1);

            // ---- what the last step left in the queue leaves the slot; then this step's text goes in ----
            if (q_tail != q_head) {
                const uint32_t n_left = q_tail - q_head;
                derive(st_n, n_left);
                st_n += n_left;
            }
            q_head = q_tail = 0;
            const uint32_t slot = tb;                             // wave-uniform
            const uint32_t my_text = slot + 16u + lane * P;       // LDS address of this lane's first byte
            posbias = rbias + off;
#pragma unroll
            for (int q = 0; q < Q; ++q)
                *reinterpret_cast<lds4_u32x4 *>(static_cast<uintptr_t>(my_text + 16u * q)) = g4_u32x4_t{cur[q].x, cur[q].y, cur[q].z, cur[q].w};
            if (lane == 0) {
                *reinterpret_cast<lds4_u32 *>(static_cast<uintptr_t>(slot + 12u)) = tail4;
                *reinterpret_cast<lds4_u32x4 *>(static_cast<uintptr_t>(slot + 16u + SB)) = g4_u32x4_t{pf0[0].x, pf0[0].y, pf0[0].z, pf0[0].w};
            }
            tail4 = __builtin_amdgcn_readlane(cur[Q - 1].w, 63);

            // ---- byte classes of this lane's P positions plus K to the left ----
            uint32_t kx[K + P];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const uint32_t w[4] = {cur[q].x, cur[q].y, cur[q].z, cur[q].w};
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                    kx[K + 16 * q + b] = pin4(cls_of((w[b >> 2] >> (8 * (b & 3))) & 0xffu));
                    __builtin_assume(kx[K + 16 * q + b] < 32u);
                }
            }
            uint32_t pk = 0;
#pragma unroll
            for (int i = 0; i < K; ++i) pk |= kx[P + i] << (8 * i);  // this lane's last K classes, oldest low
            const uint32_t left = wave_shr1_4(pk, carry);
            carry = __builtin_amdgcn_readlane(pk, 63);
#pragma unroll
            for (int i = 0; i < K; ++i) { kx[i] = (left >> (8 * i)) & 0xffu; __builtin_assume(kx[i] < 32u); }

            // ---- M words of the K-grams ending at j = 0 .. P-1 (the one ending at -1 comes from the lane to the left) ----
            uint32_t H = 0, ccnt = cnt32, roll = 0, mprev = 0;   // (the count sums go straight onto the region's count)
#pragma unroll
            for (int grp = 0; grp < P / GS; ++grp) {
                uint32_t mw[GS];
                uint32_t qe = 0;   // K = 3: the even position's 4 c_j + 4 C c_(j-1) + offM, which the odd one behind it multiplies (gram4_index.hpp)
#pragma unroll
                for (int jj = 0; jj < GS; ++jj) {
                    const int j = grp * GS + jj;
                    uint32_t x;
                    if (K == 3 && (jj & 1)) {
                        x = g4i_odd(qe, kx[K + j], offM1, C);                             // C q + (4 c_j + offM - C offM): v_lshl_add_u32, v_mad_u32_u24
                    } else if (K == 3) {
                        const G4Idx e = g4i_even(kx[K + j], kx[K + j - 1], kx[K + j - 2], offM, C);   // v_lshl_add_u32, two v_mad_u32_u24
                        x = e.addr;
                        qe = e.q;
                    } else {
                        x = pin4((kx[K + j] << 2) + offM);                                // 4 c_j + offM              (v_lshl_add_u32)
                        x = mad24(kx[K + j - 1], C4, x);                                  // + 4 C c_(j-1)             (v_mad_u32_u24)
                    }
                    mw[jj] = lds_u32(x);
                }
#pragma unroll
                for (int jj = 0; jj < GS; ++jj) {
                    const int j = grp * GS + jj;
                    roll = __builtin_amdgcn_alignbit(roll, mw[jj], 30);               // two count bits per position
                    // the hit bit of position j enters at the top: after the step's P - 1 shifts it sits at bit 32 - P + j
                    if (j > 0) H = __builtin_amdgcn_alignbit((jj == 0 ? mprev : mw[jj - 1]) >> kx[K + j], H, 1);   // (v_lshrrev_b32, v_alignbit_b32)
                    if ((j & 15) == 15) {  // 16 positions rolled in: sum the two-bit fields
                        // (each field counts once, its high bit once more: v_and_b32 and two v_bcnt_u32_b32 with the sum as their addend — round 11;
                        // low and high bits masked apart and the high count doubled took five.  Pinned: the compiler otherwise counts onto 0 and adds up)
                        ccnt = pin4(__popc(roll) + ccnt);
                        ccnt = pin4(__popc(roll & 0xaaaaaaaau) + ccnt);
                        roll = 0;
                    }
                }
                mprev = mw[GS - 1];
            }
            {   // position 0 against the M word of the K-gram ending just before this lane's share
                const uint32_t mleft = wave_shr1_4(mprev, mcarry);
                mcarry = __builtin_amdgcn_readlane(mprev, 63);
                H |= __builtin_amdgcn_ubfe(mleft, kx[K], 1) << (32 - P);
            }
            cnt32 = ccnt;

            // ---- queue the hits: a wave prefix sum of the lanes' hit counts gives each lane the list index of its first one, every lane
            // then writes its own in turns (5 VALU a turn; one ballot, two mbcnt and the slot's address in every turn cost 9 before), and
            // batches of 64 are cut from the list once the step's hits are in.  A pass queues what fits; the rest waits for the next ----
            // (list entries are LDS addresses of byte p - 3, 16 bits: my_text - 3 less the hit bit's place in H.  From the pinned lane offset, not
            // from my_text: that form took two VGPRs more at 16 positions per lane, 65, and with them the second workgroup of a CU)
            static_assert(P == 16 * Q, "lane_off = lane * 16 Q is this lane's offset in the step: my_text = tb + 16 + lane_off");
            const uint32_t text_adj = tb + (lane_off - (32u - P) + 13u);
            for (;;) {
                if (__ballot(H != 0u) == 0) break;   // (sparse text: most steps have no hit and skip the scan)
                const uint32_t n = __popc(H);
                const uint32_t incl = g4_wave_scan(n);
                const uint32_t tot = __builtin_amdgcn_readlane(incl, 63);
                const uint32_t first = q_tail + incl - n;   // list index of this lane's first hit
                const uint32_t room = first < kList4 ? kList4 - first : 0u;
                const uint32_t lim = n < room ? n : room;   // hits this lane queues in this pass (the rest stay in H)
                const uint32_t at = pin4(listb + (first << 1));   // (pinned: the compiler would add the base again inside every turn)
                g4_turns([&](auto tc) -> bool {   // turn t: the lanes with more than t hits to queue write their next one at `at` + 2 t
                    constexpr uint32_t t = decltype(tc)::value;
                    const bool w = t < lim;
                    if (__ballot(w) == 0) return false;
                    if (w) {
                        *reinterpret_cast<lds4_u16 *>(static_cast<uintptr_t>(at + 2u * t)) = static_cast<uint16_t>(text_adj + __builtin_ctz(H));
                        H &= H - 1u;
                    }
                    return true;
                }, std::make_integer_sequence<int, P>{});
                const uint32_t in = std::min(tot, kList4 - q_tail);
                q_tail += in;
                process_full();
                if (in == tot) break;
                // more hits than the list holds: the fewer than 64 entries left move to its front and the scan runs again
                const uint32_t n_left = q_tail - q_head;
                if (lane < n_left) {
                    const uint16_t v = *reinterpret_cast<lds4_cu16 *>(static_cast<uintptr_t>(listb + ((q_head + lane) << 1)));
                    *reinterpret_cast<lds4_u16 *>(static_cast<uintptr_t>(listb + (lane << 1))) = v;
                }
                q_head = 0;
                q_tail = n_left;
            }
        }
        tot_cnt += cnt32;  // per region: 32 bits cannot overflow within one
        cnt32 = 0;
        region = region_next;
        if (!(region < nregions && static_cast<uint32_t>(region_of(region).base >> 31) == slab_hi)) break;
        if constexpr (AHEAD) fetch_ahead(region);
      }
      if (st_n + q_tail - q_head != 0) process_batch(st_n + q_tail - q_head);
      if (FILT && sb_n != 0) { survivors_ask(sb_n); sb_n = 0; }
      consume_pending();
      finish_second();
      drain();
      tot_cnt += cnt32;
      cnt32 = 0;
      if constexpr (AHEAD) if (region < nregions) fetch_ahead(region);   // (the next epoch's first region)
    }
    g4_reduce(tot_cnt, reinterpret_cast<unsigned long long *>(smem), a.claim, a.result);
}

// One kernel, the variants inside: the workgroup stages M, decides TAIL (a.sel_want: 0 / 1, or 2 = by its own density probe), stages the
// directory that goes with the choice and runs the body compiled for it (gram3_kernels.hip: two launches with a probe kernel in front
// cost 60-90 us per scan, a run-time TAIL flag inside one body 10 % of the kernel).  FILT: a workgroup whose text is not made of
// dictionary words takes [coarse directory | Bloom array] in the place of the per-word directory and runs the body with the filter.
template <int K, int Q, bool ARITH, int DIR, int TPB, bool FILT, bool MPH = false>
__global__ __launch_bounds__(TPB) void gram4_kernel(const Gram4Dev g, const GramArgs a, const Gram4Lds L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int DIRC = DIR == 0 ? 1 : DIR;   // the coarse directory that goes with the filter (a per-word directory exists only beside u16 entries)
    if (!ARITH) g4_copy(smem + L.off_cls, g.cls, 256);
    g4_copy(smem + L.off_m, g.m, g.m_bytes);
    uint32_t *votes = reinterpret_cast<uint32_t *>(smem + L.off_wave);  // (the first wave's text slot: not in use yet)
    if (threadIdx.x == 0) *votes = 0;
    __syncthreads();
    // tables are read through absolute LDS addresses (this kernel has no static LDS: the dynamic segment starts at 0)
    if (__builtin_amdgcn_groupstaticsize() != 0) __builtin_trap();
    bool tail = a.sel_want == 1u;
    if (a.sel_want == 2u) {
        const uint64_t span = a.vlen > a.lead + 16 ? a.vlen - a.lead - 8 : 0;
        bool go = false;
        if (span != 0) {
            unsigned long long h = (static_cast<unsigned long long>(threadIdx.x) + 1) * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
            const uint64_t p = a.lead + 3 + (h % (span - 3));  // hit byte; p - 3 .. p + 1 lie inside the haystack
            const uint8_t *t = a.hay_al + p;
            const uint32_t OTH = g.C - 1u;
            auto cl = [&](uint32_t b) -> uint32_t {
                if (ARITH) { const uint32_t u = b - g.lo; return u < OTH ? u : OTH; }
                return reinterpret_cast<const uint8_t *>(smem + L.off_cls)[b];
            };
            const uint32_t *m = reinterpret_cast<const uint32_t *>(smem + L.off_m);
            const uint32_t c0 = cl(t[-3]), c1 = cl(t[-2]), c2 = cl(t[-1]), d = cl(t[0]), k1 = cl(t[1]);
            const uint32_t ctx = K == 3 ? (c0 * g.C + c1) * g.C + c2 : c1 * g.C + c2;
            const uint32_t w = m[ctx];
            if ((w >> d) & 1u & (d < OTH ? 1u : 0u)) {
                // (the directory is not staged yet — which one depends on this probe —: its entry comes from device memory)
                uint32_t rank = __popc(w & ((1u << d) - 1u));
                for (uint32_t j = ctx & ~3u; j < ctx; ++j) rank += __popc(m[j] & 0x3fffffffu);
                rank += g.s16 ? reinterpret_cast<const uint16_t *>(g.sdir)[ctx >> 2] : reinterpret_cast<const uint32_t *>(g.sdir)[ctx >> 2];
                const uint2 r = g.dhit_c[rank];
                go = ((r.x >> k1) & 1u) != 0;
            }
        }
        const unsigned long long bm = __ballot(go);
        if ((threadIdx.x & 63) == 0 && bm != 0) atomicAdd(votes, static_cast<uint32_t>(__popcll(bm)));
        __syncthreads();
        tail = *votes * 100u > static_cast<uint32_t>(TPB) * kProbePercent4;
        __syncthreads();
    }
    if (FILT && !tail) {
        g4_copy(smem + L.off_s, MPH ? static_cast<const void *>(g.mph_disp) : g.sdir, L.s_bytes_f);
        g4_copy(smem + L.off_b, g.bloom, g.bloom_words * 4u);
    } else {
        g4_copy(smem + L.off_s, DIR == 0 ? static_cast<const void *>(g.rfull) : g.sdir, L.s_bytes);
    }
    __syncthreads();
    if (tail) gram4_body<K, Q, ARITH, DIR, true, false>(g, a, L, smem);
    else if constexpr (FILT) gram4_body<K, Q, ARITH, DIRC, false, true, MPH>(g, a, L, smem);
    else gram4_body<K, Q, ARITH, DIR, false, false>(g, a, L, smem);
}

template <int K, int Q, bool ARITH, int DIR, int TPB, bool FILT, bool MPH = false>
static hipError_t launch4_inst(const Gram4Dev &dev, const GramArgs &a, const Gram4Lds &L, uint32_t blocks, hipStream_t stream) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gram4_kernel<K, Q, ARITH, DIR, TPB, FILT, MPH>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(L.lds_bytes));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((gram4_kernel<K, Q, ARITH, DIR, TPB, FILT, MPH>), dim3(blocks), dim3(TPB), L.lds_bytes, stream, dev, a, L);
    return hipGetLastError();
}
template <int K, int Q, int TPB, bool ARITH>
static hipError_t launch4_d(const Gram4Dev &dev, const GramArgs &a, const Gram4Lds &L, uint32_t blocks, hipStream_t stream) {
    if (L.filter && L.mph) {   // (the FILT body with the hash reads no directory: one instance per TAIL directory the other workgroups may stage)
        if (L.dir == 0) return launch4_inst<K, Q, ARITH, 0, TPB, true, true>(dev, a, L, blocks, stream);
        if (L.dir == 1) return launch4_inst<K, Q, ARITH, 1, TPB, true, true>(dev, a, L, blocks, stream);
        return launch4_inst<K, Q, ARITH, 2, TPB, true, true>(dev, a, L, blocks, stream);
    }
    if (L.filter) {
        if (L.dir == 0) return launch4_inst<K, Q, ARITH, 0, TPB, true>(dev, a, L, blocks, stream);
        if (L.dir == 1) return launch4_inst<K, Q, ARITH, 1, TPB, true>(dev, a, L, blocks, stream);
        return launch4_inst<K, Q, ARITH, 2, TPB, true>(dev, a, L, blocks, stream);
    }
    if (L.dir == 0) return launch4_inst<K, Q, ARITH, 0, TPB, false>(dev, a, L, blocks, stream);
    if (L.dir == 1) return launch4_inst<K, Q, ARITH, 1, TPB, false>(dev, a, L, blocks, stream);
    return launch4_inst<K, Q, ARITH, 2, TPB, false>(dev, a, L, blocks, stream);
}
template <int K, int Q, int TPB>
static hipError_t launch4_k(const Gram4Dev &dev, const GramArgs &a, const Gram4Lds &L, uint32_t blocks, hipStream_t stream) {
    return L.arith ? launch4_d<K, Q, TPB, true>(dev, a, L, blocks, stream) : launch4_d<K, Q, TPB, false>(dev, a, L, blocks, stream);
}

// LDS plan of a gram4 launch of `waves` waves per workgroup with `ppl` positions per lane and step:
// [hit queues | one text slot per wave | class table (256 B, when the classes are not arithmetic) | rank directory | M].
// `rfull`: the per-word directory (false: one entry per four words).  `want_filter`: the directory's place is made large enough for
// [coarse directory | Bloom array] — [displacement table of the perfect hash | Bloom array] where the handle has one (gram4_mph.hpp) — as well, for the workgroups that run the body with the filter (gram4_filter.hpp) — not taken when the
// array was not built or does not fit this shape.  Returns false when the directory asked for is not there or the tables and the
// per-wave areas do not fit — it never hands back another shape than the one asked for.
bool gram4_plan(const Gram4Dev &dev, uint32_t ppl, uint32_t waves, bool rfull, bool want_arith, bool want_filter, uint32_t lds_limit, Gram4Lds &L) {
    L = Gram4Lds{};
    if (rfull && dev.rfull == nullptr) return false;
    const uint32_t slot = 64u * ppl + 32u;
    L.wave_stride = slot;
    L.off_wave = waves * kList4 * 2u;      // the hit lists sit at 0
    L.threads = waves * 64u;
    L.arith = (want_arith && dev.arith) ? 1u : 0u;
    const uint32_t per_wg = L.off_wave + waves * L.wave_stride;
    L.off_cls = per_wg;
    L.off_s = per_wg + (L.arith ? 0u : 256u);
    L.dir = rfull ? 0u : (dev.s16 ? 1u : 2u);
    L.s_bytes = rfull ? dev.rfull_bytes : dev.s_bytes;
    uint32_t region = L.s_bytes;
    if (want_filter && dev.bloom != nullptr) {
        // (hash or rank is the upload's decision — the Bloom array was sized for the one it took —: a handle that has the hash runs it)
        const uint32_t front = dev.mph_disp != nullptr ? dev.mph_bytes : dev.s_bytes;
        const uint32_t with = front + dev.bloom_words * 4u;
        if (L.off_s + std::max(region, with) + dev.m_bytes <= lds_limit) {
            L.filter = 1u;
            L.mph = dev.mph_disp != nullptr ? 1u : 0u;
            L.s_bytes_f = front;
            L.off_b = L.off_s + front;
            region = std::max(region, with);
        }
    }
    L.off_m = L.off_s + region;
    L.lds_bytes = L.off_m + dev.m_bytes;
    return L.lds_bytes <= lds_limit;
}

// a.sel_want: 0 = plain records, 1 = tail records from the hit record on, 2 = every workgroup decides by its density probe
hipError_t launch_gram4_scan(const Gram4Dev &dev, const GramArgs &a, const Gram4Lds &L, uint32_t blocks, hipStream_t stream) {
    if (a.ppl == 32 && L.threads == 1024)
        return dev.K == 3 ? launch4_k<3, 2, 1024>(dev, a, L, blocks, stream) : launch4_k<2, 2, 1024>(dev, a, L, blocks, stream);
    if (a.ppl == 32)
        return dev.K == 3 ? launch4_k<3, 2, 512>(dev, a, L, blocks, stream) : launch4_k<2, 2, 512>(dev, a, L, blocks, stream);
    if (L.threads == 512)
        return dev.K == 3 ? launch4_k<3, 1, 512>(dev, a, L, blocks, stream) : launch4_k<2, 1, 512>(dev, a, L, blocks, stream);
    return dev.K == 3 ? launch4_k<3, 1, 1024>(dev, a, L, blocks, stream) : launch4_k<2, 1, 1024>(dev, a, L, blocks, stream);
}

}  // namespace daac
