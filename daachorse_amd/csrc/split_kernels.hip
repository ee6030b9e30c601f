// split_batch for gfx950 (daac_split_batch, daac_split, daac_offsets_compose): the word starts of a batch of documents as a streaming
// pass with one lane per byte, a bit mask and a compaction.  split.hpp has the scratch layout, include/daachorse_amd.h the definition.
//
//   marks    one lane per document: a non-empty document sets the bit of its first position (an empty one shares the bit of the
//            document behind it), the lane behind the last document sets bit `total`.  Device-scope atomicOr on 32-bit words.
//   flags    a workgroup takes a tile of kSplitTile positions.  It stages the tile's bytes with kSplitBack bytes in front and
//            kSplitAhead - 1 behind, and the tile's mark bits with a word on either side, in LDS.  A lane takes a position: the mark
//            bits around it say how many of the staged bytes belong to its document (split_reach), and split_start decides from
//            those bytes alone whether a word starts there.  One wave ballot makes one 64-bit word of the mask; the set bits of the
//            tile go to counts[tile], whose exclusive sum ranks the word starts.
//   scatter  rank = counts[tile] + the set bits of the tile's earlier mask words + those below the lane's bit; word_offsets[rank] =
//            base + position.  One lane per document looks up the rank of its first position the same way: doc_words.
//
// The local form of the rules that split_start evaluates, over the units u[i] of a document of n units and their classes c[i]:
//   AS(i): u[i] is ' and (i == 0, or c[i-1] is L or N, or c[i-1] is S and u[i-1] is not 0x20).
//   K(i):  0 unless AS(i); 2 if the bytes at i are 's 't 'm 'd; 3 if they are 're 've 'll; else 0.
//   start(0) is true; for i > 0 the first case that applies decides:
//     1. c[i] is S and c[i-1] is S: start iff i + 1 < n and c[i+1] is not S
//     2. c[i] is S: start                     3. c[i-1] is S: start iff u[i-1] is not 0x20
//     4. c[i] is L and (K(i-1) != 0 or K(i-2) == 3): no start
//     5. K(i-2) == 2 or K(i-3) == 3: start   6. otherwise: start iff c[i] != c[i-1]
//   DAAC_SPLIT_WHITESPACE: start(i) iff (c[i] is S) != (c[i-1] is S).
//   DAAC_SPLIT_BERT: start(i) iff (c[i] is S) != (c[i-1] is S), or c[i] is O, or c[i-1] is O.
// A contraction is ASCII, so K is looked up by bytes: the farthest byte read is the unit in front of a ' three bytes back (7 bytes),
// the farthest ahead the unit behind a whitespace unit (4 + 4 bytes).
//
// Reads stay inside [offsets[0], offsets[n]): a staged byte outside it is 0 and no decision reads it, because position 0 and position
// `total` carry marks.  Writes: masks and counts by the lane that owns them, word_offsets[rank] guarded by the total.
//
// DAAC_SPLIT_CL100K and DAAC_SPLIT_LLAMA3 take another flag pass behind two passes of their own (sum, carry): their local form and the
// segmented scans it reads are stated further down, in front of their functions.  The two rules above launch none of it.
// DAAC_SPLIT_O200K has three passes of the same shape with kernels of its own (an automaton scanned forwards, two bits backwards),
// stated behind those.
//
// The per-position functions below are plain C++: with DAAC_SPLIT_HOST defined this file compiles without HIP and a host program
// evaluates them at every position of documents held in buffers of exactly their size (tests/native/split_check.cpp, for the scans
// tests/native/split_rules_check.cpp, for DAAC_SPLIT_BERT and split_word_space tests/native/split_bert_check.cpp, for DAAC_SPLIT_O200K
// tests/native/split_o200k_check.cpp, under ASan and UBSan).
#ifndef DAAC_SPLIT_HOST
#include <hip/hip_runtime.h>
#define SPLIT_FN static __device__ __forceinline__
#else
#define SPLIT_FN static inline
#endif

#include <cstdint>

#include "split.hpp"
#include "../../include/daachorse_amd.h"

namespace daac {

// The bytes of the unit that begins at q, of whose document `avail` >= 1 bytes from q on may be read: 2 .. 4 for a well-formed
// sequence (Unicode Table 3-7) that fits, else 1.
SPLIT_FN int split_unit_len(const uint8_t *q, int avail) {
    const uint32_t b0 = q[0];
    if (b0 < 0xC2u || b0 > 0xF4u) return 1;
    int need;
    uint32_t lo = 0x80u, hi = 0xBFu;
    if (b0 < 0xE0u) need = 2;
    else if (b0 < 0xF0u) { need = 3; if (b0 == 0xE0u) lo = 0xA0u; if (b0 == 0xEDu) hi = 0x9Fu; }
    else { need = 4; if (b0 == 0xF0u) lo = 0x90u; if (b0 == 0xF4u) hi = 0x8Fu; }
    if (avail < need) return 1;
    if (q[1] < lo || q[1] > hi) return 1;
    for (int k = 2; k < need; ++k)
        if ((q[k] & 0xC0u) != 0x80u) return 1;
    return need;
}

// The bytes of the unit that ends in front of the unit start s, of whose document `before` >= 1 bytes in front of s may be read
// (all of them when fewer than 4).
SPLIT_FN int split_prev_len(const uint8_t *s, int before) {
    if ((s[-1] & 0xC0u) != 0x80u) return 1;
    for (int k = 2; k <= 4 && k <= before; ++k)
        if (split_unit_len(s - k, k) == k) return k;
    return 1;
}

// The class of the unit of `len` bytes at q.
SPLIT_FN uint32_t split_class(const SplitTable &t, const uint8_t *q, int len) {
    const uint32_t b0 = q[0];
    if (len == 1) {
        if ((b0 | 0x20u) - 'a' < 26u) return kSplitL;
        if (b0 - '0' < 10u) return kSplitN;
        if (b0 == 0x20u || b0 - 0x09u < 5u) return kSplitS;
        return kSplitO;
    }
    uint32_t cp;
    if (len == 2) cp = (b0 & 0x1Fu) << 6 | (q[1] & 0x3Fu);
    else if (len == 3) cp = (b0 & 0x0Fu) << 12 | (q[1] & 0x3Fu) << 6 | (q[2] & 0x3Fu);
    else cp = (b0 & 0x07u) << 18 | (q[1] & 0x3Fu) << 12 | (q[2] & 0x3Fu) << 6 | (q[3] & 0x3Fu);
    const uint32_t blk = t.stage1[cp >> 8];   // (a well-formed sequence is at most U+10FFFF: inside the first stage)
    return (t.stage2[blk * kSplitBlockBytes + ((cp & 255u) >> 2)] >> (2u * (cp & 3u))) & 3u;
}

// K of the ' at w - back (back in 1 .. 3): `before` bytes in front of w and `ahead` from w on belong to the document.
SPLIT_FN int split_contraction(const SplitTable &t, const uint8_t *w, int back, int before, int ahead) {
    if (back > before) return 0;
    const uint8_t *q = w - back;
    if (q[0] != '\'') return 0;
    const int avail = ahead + back;
    int k = 0;
    if (avail >= 2 && (q[1] == 's' || q[1] == 't' || q[1] == 'm' || q[1] == 'd')) k = 2;
    else if (avail >= 3 && ((q[1] == 'r' && q[2] == 'e') || (q[1] == 'v' && q[2] == 'e') || (q[1] == 'l' && q[2] == 'l'))) k = 3;
    if (!k || back == before) return k;   // (the document's first unit: AS holds)
    const int pl = split_prev_len(q, before - back);
    const uint32_t pc = split_class(t, q - pl, pl);
    if (pc == kSplitL || pc == kSplitN) return k;
    return pc == kSplitS && q[-1] != 0x20u ? k : 0;   // (a unit whose last byte is 0x20 is the space)
}

// Whether a word starts at the byte w.  Of w's document the bytes w[-before .. ahead - 1] may be read: before = min(bytes in front of
// w, kSplitBack), ahead = min(bytes from w to the document's end, kSplitAhead) >= 1.
SPLIT_FN bool split_start(const SplitTable &t, const uint8_t *w, int before, int ahead, int rule) {
    if ((w[0] & 0xC0u) == 0x80u)   // inside a well-formed sequence: no unit starts here
        for (int k = 1; k <= 3 && k <= before; ++k)
            if (split_unit_len(w - k, ahead + k) > k) return false;
    if (before == 0) return true;
    const int len0 = split_unit_len(w, ahead);
    const uint32_t c0 = split_class(t, w, len0);
    const int len1 = split_prev_len(w, before);
    const uint32_t c1 = split_class(t, w - len1, len1);
    const bool s0 = c0 == kSplitS, s1 = c1 == kSplitS;
    if (rule == DAAC_SPLIT_WHITESPACE) return s0 != s1;
    if (rule == DAAC_SPLIT_BERT) return s0 != s1 || c0 == kSplitO || c1 == kSplitO;
    if (s0 && s1) {
        if (len0 >= ahead) return false;
        const int len2 = split_unit_len(w + len0, ahead - len0);
        return split_class(t, w + len0, len2) != kSplitS;
    }
    if (s0) return true;
    if (s1) return w[-1] != 0x20u;
    const int k2 = split_contraction(t, w, 2, before, ahead);
    if (c0 == kSplitL && (k2 == 3 || split_contraction(t, w, 1, before, ahead) != 0)) return false;
    if (k2 == 2 || split_contraction(t, w, 3, before, ahead) == 3) return true;
    return c0 != c1;
}

// Whether the word [begin, end) of `text` is whitespace: it is not empty and its first unit, taken inside the word, is of class S.
SPLIT_FN uint8_t split_word_space(const SplitTable &t, const uint8_t *text, uint64_t begin, uint64_t end) {
    if (end <= begin) return 0;
    const int avail = end - begin < 4 ? static_cast<int>(end - begin) : 4;
    const uint8_t *q = text + begin;
    return split_class(t, q, split_unit_len(q, avail)) == kSplitS ? 1 : 0;
}

// before and ahead of a position from the mark bits around it: bit k of `win` is the mark of position p - kSplitBack + k,
// k < kSplitBack + kSplitAhead.  A mark at or in front of p ends the look-back, a mark behind p the look-ahead.
SPLIT_FN void split_reach(uint32_t win, int &before, int &ahead) {
    const uint32_t back = win & ((2u << kSplitBack) - 2u);   // positions p - kSplitBack + 1 .. p
    before = back ? kSplitBack - (31 - __builtin_clz(back)) : kSplitBack;
    const uint32_t fwd = (win >> (kSplitBack + 1)) & ((1u << (kSplitAhead - 1)) - 1u);   // positions p + 1 .. p + kSplitAhead - 1
    ahead = fwd ? __builtin_ctz(fwd) + 1 : kSplitAhead;
}

// ------------------------------------------------------------------------------- DAAC_SPLIT_CL100K and DAAC_SPLIT_LLAMA3: the scans
// The local form of the two rules (include/daachorse_amd.h has the patterns), over units u[i] with classes c[i]; nl(i): u[i] is 0x0A or
// 0x0D; sp(i): u[i] is 0x20.  Four quantities depend on runs of any length, none of which crosses a document boundary:
//   D(i), c[i] is N: the index of i in its maximal run of N units.
//   T(i), nl(i):     the maximal run of nl units that ends at i has an O unit directly in front of it.
//   F(i), c[i] is S: an nl unit lies behind i in the same maximal run of S units.
//   E(i), c[i] is S: the maximal S run that holds i reaches the document's end (read by cl100k alone).
//   sO(j): j == 0, or c[j-1] is L or N, or c[j-1] is S and not sp(j-1).
//   K(j):  0 unless u[j] is ' and sO(j); 2 if u[j+1] folds to s t m d; 3 if u[j+1..j+2] fold to re ve ll; else 0.  Folding: an ASCII
//          letter in either case, and U+017F for s where the table has it in class L.
//   start(0) is true; for i > 0 the first case that applies decides:
//     c[i] is N: start iff D(i) % 3 == 0
//     c[i] is S: 1. nl(i) and T(i): no start           2. c[i-1] is not S, or nl(i-1) and T(i-1): start
//                3. cl100k only, E(i): no start        4. nl(i): no start      5. F(i): no start      6. nl(i-1): start
//                7. start iff i + 1 < n and c[i+1] is not S
//     c[i] is L: 1. K(i-1) != 0 or K(i-2) == 3: no start                       2. K(i-2) == 2 or K(i-3) == 3: start
//                3. c[i-1] is L: no start   4. c[i-1] is N: start   5. c[i-1] is S: start iff nl(i-1)
//                6. c[i-1] is O: start iff not sO(i-1)
//     c[i] is O: start iff sO(i)
// The farthest byte read is the unit in front of a ' three bytes back (7 bytes), the farthest ahead the unit behind a whitespace unit.
//
// The scans run over positions, not units: every byte of a unit carries its unit's class ("filled"), so a run of units is a run of
// positions, and a unit that straddles a tile edge needs nothing special.  Each is a state that a position either keeps or sets:
//   y (forwards, mod 3): the unit starts of the N run up to and including p.  Set to 0 where p is not N, to 1 where a document starts
//     at p; a unit start adds 1.  D(i) % 3 == 0 iff y == 1 at i's first byte.
//   x (forwards): set to 1 at an O position, kept at an nl position that starts no document, else set to 0.  T(i) = nl(i) and x.
//   f (backwards): set to 1 at an nl position, kept at another S position with no document start behind it, else set to 0.  F(i) = f
//     at a position that is not nl.
//   e (backwards): set to 1 at an S position with a document start (or the text's end) behind it, kept at another S position, else 0.
// A word of 64 positions is eight masks (SplitPlanes); what it does to the four states is a packed function (kSum*, split.hpp), found
// with count-leading and count-trailing zeros; functions compose (split_sum_then), so a tile, and a span of tiles, is a function too.
//   sum     a workgroup per tile: the predicate bits by ballot, the words' functions, composed into tile_sum[tile].
//   carry   one workgroup: a lane composes a span of tiles, lane 0 walks the kSplitCarryLanes spans, each lane walks its span again
//           and writes carry_f (forwards) and carry_b (backwards).  No lane waits for another workgroup.
//   flags   as for GPT-2, with the masks built again and the state of a position read from its word's masks and the word's carries.
// The work at a position does not depend on the length of the run it lies in.

struct SplitPlanes {
    uint64_t un;    // a unit of class N starts here
    uint64_t nkd;   // y is set here: not N, or a document starts here
    uint64_t nkt;   // x is set here: not an nl that starts no document
    uint64_t o;     // class O: what x is set to
    uint64_t nkf;   // f is set here
    uint64_t nl;    // nl: what f is set to
    uint64_t nke;   // e is set here
    uint64_t ve;    // S with a document start behind it: what e is set to
};

enum : uint32_t { kPredU = 1, kPredN = 2, kPredS = 4, kPredNl = 8, kPredO = 16 };

// The predicate bits of the byte w: whether a unit starts there, the class of the unit that holds it, and nl.  before and ahead as for
// split_start.
SPLIT_FN uint32_t split_pred(const SplitTable &t, const uint8_t *w, int before, int ahead) {
    const uint8_t *q = w;
    int len = 0;
    if ((w[0] & 0xC0u) == 0x80u)
        for (int k = 1; k <= 3 && k <= before; ++k) {
            const int n = split_unit_len(w - k, ahead + k);
            if (n > k) { q = w - k; len = n; break; }
        }
    uint32_t bits = 0;
    if (!len) { len = split_unit_len(w, ahead); bits = kPredU; }
    const uint32_t c = split_class(t, q, len);
    if (c == kSplitN) return bits | kPredN;
    if (c == kSplitO) return bits | kPredO;
    if (c == kSplitL) return bits;
    return bits | kPredS | (w[0] == 0x0Au || w[0] == 0x0Du ? kPredNl : 0u);
}

// The masks of a word from the ballots of its positions: mark is "a document starts here", mark1 the same one position on.
SPLIT_FN SplitPlanes split_planes(uint64_t u, uint64_t n, uint64_t s, uint64_t nl, uint64_t o, uint64_t mark, uint64_t mark1) {
    SplitPlanes p;
    p.un = u & n;
    p.nkd = ~n | mark;
    p.nkt = ~(nl & ~mark);
    p.o = o;
    p.nkf = ~(s & ~nl & ~mark1);
    p.nl = nl;
    p.nke = ~(s & ~mark1);
    p.ve = s & mark1;
    return p;
}

SPLIT_FN uint32_t split_mod3(uint32_t v) { return v % 3u; }
SPLIT_FN uint64_t split_low(uint32_t k) { return (2ull << k) - 1ull; }   // bits 0 .. k, k < 64

// What a word does to the four states.
SPLIT_FN uint32_t split_word_sum(const SplitPlanes &p) {
    uint32_t r = 0;
    if (!p.nkd) r |= kSumKeepD | split_mod3(static_cast<uint32_t>(__builtin_popcountll(p.un))) << 1;
    else r |= split_mod3(static_cast<uint32_t>(__builtin_popcountll(p.un & (~0ull << (63 - __builtin_clzll(p.nkd)))))) << 1;
    if (!p.nkt) r |= kSumKeepT;
    else if ((p.o >> (63 - __builtin_clzll(p.nkt))) & 1ull) r |= kSumValT;
    if (!p.nkf) r |= kSumKeepF;
    else if ((p.nl >> __builtin_ctzll(p.nkf)) & 1ull) r |= kSumValF;
    if (!p.nke) r |= kSumKeepE;
    else if ((p.ve >> __builtin_ctzll(p.nke)) & 1ull) r |= kSumValE;
    return r;
}

// The function "first, then second" (for the backward states `first` is the part that lies behind).
SPLIT_FN uint32_t split_sum_then(uint32_t first, uint32_t second) {
    uint32_t r;
    if (second & kSumKeepD) r = (first & kSumKeepD) | split_mod3(((first & kSumAddD) >> 1) + ((second & kSumAddD) >> 1)) << 1;
    else r = second & kSumAddD;
    r |= (second & kSumKeepT ? first : second) & (kSumKeepT | kSumValT);
    r |= (second & kSumKeepF ? first : second) & (kSumKeepF | kSumValF);
    r |= (second & kSumKeepE ? first : second) & (kSumKeepE | kSumValE);
    return r;
}

// The forward states behind a part, from those in front of it, and the backward states in front of a part, from those behind it.
SPLIT_FN uint32_t split_apply_fwd(uint32_t sum, uint32_t st) {
    const uint32_t y = split_mod3((sum & kSumKeepD ? st & 3u : 0u) + ((sum & kSumAddD) >> 1));
    const uint32_t x = sum & kSumKeepT ? (st >> 2) & 1u : (sum & kSumValT ? 1u : 0u);
    return y | x << 2;
}
SPLIT_FN uint32_t split_apply_bwd(uint32_t sum, uint32_t st) {
    const uint32_t f = sum & kSumKeepF ? st & 1u : (sum & kSumValF ? 1u : 0u);
    const uint32_t e = sum & kSumKeepE ? (st >> 1) & 1u : (sum & kSumValE ? 1u : 0u);
    return f | e << 1;
}

// What a span of parts does: the forward fields composed from its first part on, the backward fields from its last.
SPLIT_FN uint32_t split_span_sum(const uint32_t *sum, uint64_t begin, uint64_t end) {
    uint32_t f = kSumIdentity, b = kSumIdentity;
    for (uint64_t i = begin; i < end; ++i) f = split_sum_then(f, sum[i]);
    for (uint64_t i = end; i > begin; --i) b = split_sum_then(b, sum[i - 1]);
    return (f & kSumFwd) | (b & kSumBwd);
}

// The carries of the parts of a span: carry_f[i] the forward states in front of part i given f_in in front of the span, carry_b[i] the
// backward states behind part i given b_in behind the span.
SPLIT_FN void split_span_carries(const uint32_t *sum, uint64_t begin, uint64_t end, uint32_t f_in, uint32_t b_in, uint32_t *carry_f, uint32_t *carry_b) {
    for (uint64_t i = begin; i < end; ++i) { carry_f[i] = f_in; f_in = split_apply_fwd(sum[i], f_in); }
    for (uint64_t i = end; i > begin; --i) { carry_b[i - 1] = b_in; b_in = split_apply_bwd(sum[i - 1], b_in); }
}

struct SplitScan { uint32_t y, x, x_prev, f, e; };

// The states at bit k of a word: cf the forward states in front of the word, cb the backward states behind it.  x_prev is x one
// position back.
SPLIT_FN SplitScan split_scan_at(const SplitPlanes &p, uint32_t k, uint32_t cf, uint32_t cb) {
    SplitScan s;
    const uint64_t low = split_low(k), high = ~0ull << k;
    uint64_t m = p.nkd & low;
    if (!m) s.y = split_mod3((cf & 3u) + static_cast<uint32_t>(__builtin_popcountll(p.un & low)));
    else s.y = split_mod3(static_cast<uint32_t>(__builtin_popcountll(p.un & low & (~0ull << (63 - __builtin_clzll(m))))));
    m = p.nkt & low;
    s.x = m ? static_cast<uint32_t>((p.o >> (63 - __builtin_clzll(m))) & 1ull) : (cf >> 2) & 1u;
    m = p.nkt & (low >> 1);
    s.x_prev = m ? static_cast<uint32_t>((p.o >> (63 - __builtin_clzll(m))) & 1ull) : (cf >> 2) & 1u;
    m = p.nkf & high;
    s.f = m ? static_cast<uint32_t>((p.nl >> __builtin_ctzll(m)) & 1ull) : cb & 1u;
    m = p.nke & high;
    s.e = m ? static_cast<uint32_t>((p.ve >> __builtin_ctzll(m)) & 1ull) : (cb >> 1) & 1u;
    return s;
}

// The letter the unit at q folds to, as far as the contractions go (0: none of theirs); len: the unit's bytes.
SPLIT_FN uint32_t split_fold(const SplitTable &t, const uint8_t *q, int avail, int &len) {
    len = 1;
    const uint32_t b = q[0];
    if ((b | 0x20u) - 'a' < 26u) return b | 0x20u;
    if (b == 0xC5u && avail >= 2 && q[1] == 0xBFu && split_class(t, q, 2) == kSplitL) { len = 2; return 's'; }
    return 0;
}

// sO of the unit start q with `before` bytes of its document in front of it.
SPLIT_FN bool split_so(const SplitTable &t, const uint8_t *q, int before) {
    if (before <= 0) return true;
    const int pl = split_prev_len(q, before);
    const uint32_t pc = split_class(t, q - pl, pl);
    if (pc == kSplitL || pc == kSplitN) return true;
    return pc == kSplitS && q[-1] != 0x20u;
}

// K of the unit start q: `before` bytes of its document in front of it, `avail` >= 1 from q on.
SPLIT_FN int split_contraction_fold(const SplitTable &t, const uint8_t *q, int before, int avail) {
    if (q[0] != '\'' || avail < 2) return 0;
    int l1;
    const uint32_t a = split_fold(t, q + 1, avail - 1, l1);
    int k = 0;
    if (a == 's' || a == 't' || a == 'm' || a == 'd') k = 2;
    else if (a && avail >= 3) {
        const uint32_t b = q[2] | 0x20u;
        if ((a == 'r' && b == 'e') || (a == 'v' && b == 'e') || (a == 'l' && b == 'l')) k = 3;
    }
    return k && split_so(t, q, before) ? k : 0;
}

// Whether a word starts at the byte w under DAAC_SPLIT_CL100K or DAAC_SPLIT_LLAMA3; before and ahead as for split_start, s the scan
// states at w.
SPLIT_FN bool split_start_scanned(const SplitTable &t, const uint8_t *w, int before, int ahead, int rule, const SplitScan &s) {
    if ((w[0] & 0xC0u) == 0x80u)
        for (int k = 1; k <= 3 && k <= before; ++k)
            if (split_unit_len(w - k, ahead + k) > k) return false;
    if (before == 0) return true;
    const int len0 = split_unit_len(w, ahead);
    const uint32_t c0 = split_class(t, w, len0);
    if (c0 == kSplitN) return s.y == 1u;
    const int len1 = split_prev_len(w, before);
    const uint32_t c1 = split_class(t, w - len1, len1);
    const bool nl1 = w[-1] == 0x0Au || w[-1] == 0x0Du;   // (a unit that ends in such a byte is that byte)
    if (c0 == kSplitO) return c1 == kSplitL || c1 == kSplitN || (c1 == kSplitS && w[-1] != 0x20u);
    if (c0 == kSplitS) {
        const bool nl0 = w[0] == 0x0Au || w[0] == 0x0Du;
        if (nl0 && s.x) return false;
        if (c1 != kSplitS || (nl1 && s.x_prev)) return true;
        if (rule == DAAC_SPLIT_CL100K && s.e) return false;
        if (nl0 || s.f) return false;
        if (nl1) return true;
        if (len0 >= ahead) return false;
        const int len2 = split_unit_len(w + len0, ahead - len0);
        return split_class(t, w + len0, len2) != kSplitS;
    }
    // a letter: inside a contraction, behind one, or by the unit in front
    if (split_contraction_fold(t, w - 1, before - 1, ahead + 1) != 0) return false;
    const int k2 = before > len1 ? split_contraction_fold(t, w - len1 - 1, before - len1 - 1, ahead + len1 + 1) : 0;
    if (k2 == 3) return false;
    if (k2 == 2) return true;
    if (before >= 3 && split_contraction_fold(t, w - 3, before - 3, ahead + 3) == 3) return true;
    if (c1 == kSplitL) return false;
    if (c1 == kSplitN) return true;
    if (c1 == kSplitS) return nl1;
    return !split_so(t, w - len1, before - len1);
}

// ------------------------------------------------------------------------------------------- DAAC_SPLIT_O200K: the automaton and the scans
// The local form of the rule (include/daachorse_amd.h has the pattern), over units u[i] with classes c[i]: Up (Lu, Lt), Low (Ll),
// C (a caseless letter: Lm, Lo), M (a mark), N, S and O; nl(i) and sp(i) as above.  Body units are Up, Low, C and M.
//   K(j): 0 unless u[j] is '; 2 if u[j+1] folds to s t m d; 3 if u[j+1..j+2] fold to re ve ll; else 0 (folding as above, U+017F where
//         the table has it as a letter of any case).
// One forward state q(i), "the kind of match unit i lies in", is an automaton over the units, started at None in front of a document:
//   None    an S unit outside a trailer (and the document's start)
//   Pfx     a single O unit (not M) at a match start: the prefix of a word if a body unit follows, else punctuation
//   Punct   the body of the punctuation alternative             Trail   its trailer [\r\n/]*
//   Body0   word body, no Low unit since the last Up unit or the word's start           Body1   word body, a Low unit since then
//   Apos2, Apos3, Mid3, Fin   the ' of a suffix 's 't 'm 'd, the ' and the middle letter of 're 've 'll, a suffix's last letter
//   Dig1, Dig2, Dig3          the first, second and third unit of a \p{N}{1,3} match
// q(i) = next(q(i-1), cat(i)), first case that applies:
//   q(i-1) is Apos2 or Mid3: Fin           q(i-1) is Apos3: Mid3        (K has read these letters)
//   Up: Body0          Low: Body1          C: Body1 if q(i-1) is Body1, else Body0
//   M:  Punct if q(i-1) is Punct; Body1 if it is Body1; else Body0      (a mark at a match start or behind a prefix is word body)
//   N:  Dig2 behind Dig1, Dig3 behind Dig2, else Dig1
//   nl: Trail if q(i-1) is Pfx, Punct or Trail, else None               another S: None
//   ' with K(i) != 0 and q(i-1) a Body: Apos2 or Apos3
//   O:  Punct if q(i-1) is Pfx or Punct, or if sp(i-1); Trail if u[i] is / and q(i-1) is Trail; else Pfx
// Two backward bits: f as above (a newline farther on in the whitespace run), and
//   g(i), c[i] is Up: the maximal run of Up units from i on is directly followed by a unit that is not Low, C or M, or by the
//         document's end.  (U*Lw+ then backs off to the last caseless unit or mark in front of the run.)
// start(0) is true; for i > 0, with s = q(i-1), the first case that applies decides:
//   s is Apos2, Apos3 or Mid3: no start
//   c[i] is N: start iff s is not Dig1 or Dig2
//   c[i] is S: 1. nl(i) and s is Pfx, Punct or Trail: no start     2. s is not None: start       3. nl(i): no start
//              4. f(i): no start     5. nl(i-1): start             6. start iff i + 1 < n and c[i+1] is not S
//   c[i] is O: 1. K(i) != 0 and s is a Body: no start              2. s is Pfx or Punct: no start
//              3. u[i] is / and s is Trail: no start               4. start iff not sp(i-1)
//   a body unit: 1. s is a Body: no start unless c[i] is Up; then start iff s is Body1, or c[i-1] is C or M and g(i)
//              2. s is Pfx: no start       3. c[i] is M and s is Punct: no start     4. s is None: start iff nl(i-1)     5. start
// The farthest byte read is the unit in front of the position (4 bytes), the farthest ahead the unit behind a whitespace unit and the
// letters behind a ' (3 bytes).
//
// The scans run over positions as above: a byte inside a unit keeps the forward state, and carries its unit's class for the backward
// bits.  What a position does to q is a map of the 13 states to themselves, packed four bits a state (state s in bits 4 s .. 4 s + 3);
// a position that starts a document maps every state to next(None, .).  Maps compose by 13 nibble look-ups (o200k_then), so a word of
// 64 positions, a tile and a span of tiles are maps too.  What a position does to (f, g) is keep-or-set as above (two keep bits, two
// values; o200k_back_then).
//   sum     a workgroup per tile: a lane takes a position's two functions, a wave composes its 64 with shuffles (a prefix scan forwards,
//           a suffix scan backwards), the tile's 16 words are composed into tile_map[tile] and tile_sum[tile].
//   carry   one workgroup, as above: a lane composes a span of tiles, lane 0 walks the spans' states, each lane its span's.
//   flags   the wave scans again; the state in front of a position is its wave's exclusive map applied to the state in front of the word.

enum : uint32_t { kQNone = 0, kQPfx, kQPunct, kQTrail, kQBody0, kQBody1, kQApos2, kQApos3, kQMid3, kQFin, kQDig1, kQDig2, kQDig3, kO200kStates };
enum : uint32_t { kCatUp = 0, kCatLow, kCatC, kCatM, kCatN, kCatNl, kCatS, kCatO, kCatSlash, kCatOSp, kCatSlashSp, kCatApos2, kCatApos3, kO200kCats };
// what o200k_info packs: the category in bits 0 .. 3, then
enum : uint32_t { kInfoStart = 16, kInfoCaseless = 32, kInfoUp = 64, kInfoS = 128, kInfoNl = 256 };
constexpr uint64_t kO200kIdentity = 0xFEDCBA9876543210ull;
constexpr uint32_t kBackIdentity = 3u;   // (f, g) functions: keep bits 0 (f) and 1 (g), values in bits 2 and 3; the states f | g << 1

constexpr uint32_t o200k_next(uint32_t s, uint32_t cat) {
    if (s == kQApos2 || s == kQMid3) return kQFin;
    if (s == kQApos3) return kQMid3;
    const bool body = s == kQBody0 || s == kQBody1, punct = s == kQPfx || s == kQPunct;
    switch (cat) {
    case kCatUp: return kQBody0;
    case kCatLow: return kQBody1;
    case kCatC: return s == kQBody1 ? kQBody1 : kQBody0;
    case kCatM: return s == kQPunct ? kQPunct : s == kQBody1 ? kQBody1 : kQBody0;
    case kCatN: return s == kQDig1 ? kQDig2 : s == kQDig2 ? kQDig3 : kQDig1;
    case kCatNl: return punct || s == kQTrail ? kQTrail : kQNone;
    case kCatS: return kQNone;
    case kCatApos2: if (body) return kQApos2; break;
    case kCatApos3: if (body) return kQApos3; break;
    case kCatSlash: case kCatSlashSp: if (s == kQTrail) return kQTrail; break;
    default: break;
    }
    if (punct || ((cat == kCatOSp || cat == kCatSlashSp) && s == kQNone)) return kQPunct;
    return kQPfx;
}

constexpr uint64_t o200k_map_of(uint32_t cat) {
    uint64_t m = 0;
    for (uint32_t s = 0; s < kO200kStates; ++s) m |= static_cast<uint64_t>(o200k_next(s, cat)) << (4u * s);
    return m;
}
constexpr uint64_t kMapUp = o200k_map_of(kCatUp), kMapLow = o200k_map_of(kCatLow), kMapC = o200k_map_of(kCatC), kMapM = o200k_map_of(kCatM),
                   kMapN = o200k_map_of(kCatN), kMapNl = o200k_map_of(kCatNl), kMapS = o200k_map_of(kCatS), kMapO = o200k_map_of(kCatO),
                   kMapSlash = o200k_map_of(kCatSlash), kMapOSp = o200k_map_of(kCatOSp), kMapSlashSp = o200k_map_of(kCatSlashSp),
                   kMapApos2 = o200k_map_of(kCatApos2), kMapApos3 = o200k_map_of(kCatApos3);

SPLIT_FN uint64_t o200k_map(uint32_t cat) {
    switch (cat) {
    case kCatUp: return kMapUp;
    case kCatLow: return kMapLow;
    case kCatC: return kMapC;
    case kCatM: return kMapM;
    case kCatN: return kMapN;
    case kCatNl: return kMapNl;
    case kCatS: return kMapS;
    case kCatSlash: return kMapSlash;
    case kCatOSp: return kMapOSp;
    case kCatSlashSp: return kMapSlashSp;
    case kCatApos2: return kMapApos2;
    case kCatApos3: return kMapApos3;
    default: return kMapO;
    }
}

// The map "first a, then b", and the state behind a map given the state in front of it.
SPLIT_FN uint64_t o200k_then(uint64_t a, uint64_t b) {
    uint64_t r = 0;
    for (uint32_t s = 0; s < kO200kStates; ++s) r |= ((b >> (((a >> (4u * s)) & 15u) * 4u)) & 15ull) << (4u * s);
    return r;
}
SPLIT_FN uint32_t o200k_apply(uint64_t m, uint32_t st) { return static_cast<uint32_t>(m >> (4u * st)) & 15u; }

// The (f, g) function "first `behind`, then `front`" (the bits run backwards), and the bits in front of a function given those behind it.
SPLIT_FN uint32_t o200k_back_then(uint32_t behind, uint32_t front) {
    return (front & behind & 3u) | ((((front >> 2) & ~front) | ((behind >> 2) & front)) & 3u) << 2;
}
SPLIT_FN uint32_t o200k_back_apply(uint32_t fn, uint32_t st) { return (st & fn & 3u) | ((fn >> 2) & ~fn & 3u); }

// The class of the unit of `len` bytes at q under DAAC_SPLIT_O200K: the table has four bits a code point.
SPLIT_FN uint32_t o200k_class(const SplitTable &t, const uint8_t *q, int len) {
    const uint32_t b0 = q[0];
    if (len == 1) {
        if (b0 - 'A' < 26u) return kSplitUp;
        if (b0 - 'a' < 26u) return kSplitLow;
        if (b0 - '0' < 10u) return kSplitN;
        if (b0 == 0x20u || b0 - 0x09u < 5u) return kSplitS;
        return kSplitO;
    }
    uint32_t cp;
    if (len == 2) cp = (b0 & 0x1Fu) << 6 | (q[1] & 0x3Fu);
    else if (len == 3) cp = (b0 & 0x0Fu) << 12 | (q[1] & 0x3Fu) << 6 | (q[2] & 0x3Fu);
    else cp = (b0 & 0x07u) << 18 | (q[1] & 0x3Fu) << 12 | (q[2] & 0x3Fu) << 6 | (q[3] & 0x3Fu);
    const uint32_t blk = t.stage1[cp >> 8];
    return (t.stage2[blk * kSplitBlockBytes4 + ((cp & 255u) >> 1)] >> (4u * (cp & 1u))) & 15u;
}

// K of the ' at q, of whose document `avail` >= 1 bytes from q on may be read.
SPLIT_FN int o200k_suffix(const SplitTable &t, const uint8_t *q, int avail) {
    if (avail < 2) return 0;
    uint32_t a = q[1];
    if ((a | 0x20u) - 'a' < 26u) a |= 0x20u;
    else if (a == 0xC5u && avail >= 3 && q[2] == 0xBFu) {   // U+017F
        const uint32_t c = o200k_class(t, q + 1, 2);
        return c == kSplitL || c == kSplitUp || c == kSplitLow ? 2 : 0;
    } else return 0;
    if (a == 's' || a == 't' || a == 'm' || a == 'd') return 2;
    if (avail < 3) return 0;
    const uint32_t b = q[2] | 0x20u;
    return (a == 'r' && b == 'e') || (a == 'v' && b == 'e') || (a == 'l' && b == 'l') ? 3 : 0;
}

// What the byte w is under DAAC_SPLIT_O200K (kInfo*): whether a unit starts there and its category, and of the unit that holds the
// byte whether it is Up, caseless or mark, S, nl.  before and ahead as for split_start.
SPLIT_FN uint32_t o200k_info(const SplitTable &t, const uint8_t *w, int before, int ahead) {
    const uint8_t *q = w;
    int len = 0;
    if ((w[0] & 0xC0u) == 0x80u)
        for (int k = 1; k <= 3 && k <= before; ++k) {
            const int n = split_unit_len(w - k, ahead + k);
            if (n > k) { q = w - k; len = n; break; }
        }
    uint32_t bits = 0;
    if (!len) { len = split_unit_len(w, ahead); bits = kInfoStart; }
    const uint32_t c = o200k_class(t, q, len);
    switch (c) {
    case kSplitUp: return bits | kInfoUp | kCatUp;
    case kSplitLow: return bits | kCatLow;
    case kSplitL: return bits | kInfoCaseless | kCatC;
    case kSplitMark: return bits | kInfoCaseless | kCatM;
    case kSplitN: return bits | kCatN;
    case kSplitS: return bits | kInfoS | (w[0] == 0x0Au || w[0] == 0x0Du ? kInfoNl | kCatNl : kCatS);
    default: break;
    }
    const bool sp = before > 0 && w[-1] == 0x20u;   // (a unit whose last byte is 0x20 is the space)
    if (w[0] == '/') return bits | (sp ? kCatSlashSp : kCatSlash);
    if (sp) return bits | kCatOSp;
    const int k = w[0] == '\'' ? o200k_suffix(t, w, ahead) : 0;
    return bits | (k == 2 ? kCatApos2 : k == 3 ? kCatApos3 : kCatO);
}

// What a position does to the forward state: first says that a document starts there.
SPLIT_FN uint64_t o200k_fwd_of(uint32_t info, bool first) {
    if (!(info & kInfoStart)) return kO200kIdentity;
    const uint64_t m = o200k_map(info & 15u);
    return first ? (m & 15ull) * 0x1111111111111111ull : m;
}

// What a position does to (f, g): last says that a document starts, or the text ends, behind it.
SPLIT_FN uint32_t o200k_back_of(uint32_t info, bool last) {
    uint32_t keep = 0, val = 0;
    if (info & kInfoNl) val |= 1u;
    else if ((info & kInfoS) && !last) keep |= 1u;
    if ((info & kInfoUp) && !last) keep |= 2u;
    else if (info & kInfoUp) val |= 2u;
    else if ((info & 15u) != kCatLow && !(info & kInfoCaseless)) val |= 2u;
    return keep | val << 2;
}

// What a span of parts does to the forward state and to (f, g).
SPLIT_FN uint64_t o200k_span_map(const unsigned long long *map, uint64_t begin, uint64_t end) {
    uint64_t m = kO200kIdentity;
    for (uint64_t i = begin; i < end; ++i) m = o200k_then(m, map[i]);
    return m;
}
SPLIT_FN uint32_t o200k_span_back(const uint32_t *fn, uint64_t begin, uint64_t end) {
    uint32_t b = kBackIdentity;
    for (uint64_t i = end; i > begin; --i) b = o200k_back_then(b, fn[i - 1]);
    return b;
}

// The carries of the parts of a span: carry_f[i] the forward state in front of part i given f_in in front of the span, carry_b[i] the
// backward bits behind part i given b_in behind the span.
SPLIT_FN void o200k_span_carries(const unsigned long long *map, const uint32_t *fn, uint64_t begin, uint64_t end, uint32_t f_in, uint32_t b_in, uint32_t *carry_f,
                                 uint32_t *carry_b) {
    for (uint64_t i = begin; i < end; ++i) { carry_f[i] = f_in; f_in = o200k_apply(map[i], f_in); }
    for (uint64_t i = end; i > begin; --i) { carry_b[i - 1] = b_in; b_in = o200k_back_apply(fn[i - 1], b_in); }
}

// Whether a word starts at the byte w under DAAC_SPLIT_O200K; before and ahead as for split_start, info = o200k_info of the byte, s the
// forward state in front of it, back the bits f | g << 1 at it.
SPLIT_FN bool o200k_start(const SplitTable &t, const uint8_t *w, int before, int ahead, uint32_t info, uint32_t s, uint32_t back) {
    if (!(info & kInfoStart)) return false;
    if (before == 0) return true;
    if (s == kQApos2 || s == kQApos3 || s == kQMid3) return false;
    const uint32_t cat = info & 15u;
    const bool body = s == kQBody0 || s == kQBody1;
    const bool nl1 = w[-1] == 0x0Au || w[-1] == 0x0Du;   // (a unit that ends in such a byte is that byte)
    if (cat == kCatN) return s != kQDig1 && s != kQDig2;
    if (info & kInfoS) {
        const bool nl0 = (info & kInfoNl) != 0;
        if (nl0 && (s == kQPfx || s == kQPunct || s == kQTrail)) return false;
        if (s != kQNone) return true;
        if (nl0 || (back & 1u)) return false;
        if (nl1) return true;
        const int len0 = split_unit_len(w, ahead);
        if (len0 >= ahead) return false;
        const int len2 = split_unit_len(w + len0, ahead - len0);
        return o200k_class(t, w + len0, len2) != kSplitS;
    }
    if (cat >= kCatO) {
        if ((cat == kCatApos2 || cat == kCatApos3) && body) return false;
        if (s == kQPfx || s == kQPunct) return false;
        if (cat == kCatSlash && s == kQTrail) return false;
        return cat != kCatOSp && cat != kCatSlashSp;
    }
    if (body) {
        if (cat != kCatUp) return false;
        if (s == kQBody1) return true;
        if (!(back & 2u)) return false;
        const int len1 = split_prev_len(w, before);
        const uint32_t c1 = o200k_class(t, w - len1, len1);
        return c1 == kSplitL || c1 == kSplitMark;
    }
    if (s == kQPfx || (cat == kCatM && s == kQPunct)) return false;
    return s == kQNone ? nl1 : true;
}

// split_word_space under DAAC_SPLIT_O200K: the same over its table.
SPLIT_FN uint8_t o200k_word_space(const SplitTable &t, const uint8_t *text, uint64_t begin, uint64_t end) {
    if (end <= begin) return 0;
    const int avail = end - begin < 4 ? static_cast<int>(end - begin) : 4;
    const uint8_t *q = text + begin;
    return o200k_class(t, q, split_unit_len(q, avail)) == kSplitS ? 1 : 0;
}

#ifndef DAAC_SPLIT_HOST
// ------------------------------------------------------------------------------------------------------- kernels and launchers
constexpr uint32_t kSplitTileWords = kSplitTile / 64;     // mask words of a tile
constexpr uint32_t kSplitMarkWords = kSplitTile / 32;     // mark words of a tile
constexpr uint32_t kSplitMaxBlocks = 1u << 20;            // workgroups of a pass; they stride over the tiles
static_assert(kSplitTile % kSplitLanes == 0 && kSplitLanes % 64 == 0, "a wave's positions are one mask word");
static_assert(kSplitBack + kSplitAhead <= 32 && kSplitBack < 32, "the mark window is one 32-bit word");

__global__ __launch_bounds__(256) void split_mark_kernel(const SplitArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride) {
        const uint64_t off = a.doc_off[d];
        if (off < a.base || off - a.base > a.total) continue;   // (never: the driver has checked the offsets)
        const uint64_t p = off - a.base;
        if (d < a.n_docs && a.doc_off[d + 1] <= off) continue;  // an empty document
        atomicOr(&a.marks[p >> 5], 1u << (p & 31u));
    }
}

__global__ __launch_bounds__(kSplitLanes) void split_flag_kernel(const SplitArgs a) {
    __shared__ uint8_t s_txt[kSplitTile + 32];             // entry kSplitBack + l: the byte of the tile's position l
    __shared__ uint32_t s_mark[kSplitMarkWords + 2];       // entry 1 + j: the tile's mark word j
    __shared__ uint32_t s_cnt[kSplitLanes / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_mark = a.tiles * kSplitMarkWords + 1;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint64_t base = tile * kSplitTile;
        for (uint32_t i = tid; i < kSplitTile + kSplitBack + kSplitAhead - 1; i += kSplitLanes) {
            const uint64_t p = base + i;   // the position + kSplitBack
            s_txt[i] = p >= static_cast<uint64_t>(kSplitBack) && p - kSplitBack < a.total ? a.text[p - kSplitBack] : static_cast<uint8_t>(0);
        }
        for (uint32_t i = tid; i < kSplitMarkWords + 2; i += kSplitLanes) {
            const uint64_t w = tile * kSplitMarkWords + i;   // the word + 1
            s_mark[i] = w >= 1 && w - 1 < n_mark ? a.marks[w - 1] : 0u;
        }
        __syncthreads();
        uint32_t cnt = 0;
        for (uint32_t it = 0; it < kSplitTile / kSplitLanes; ++it) {
            const uint32_t l = it * kSplitLanes + tid;
            const uint64_t p = base + l;
            bool f = false;
            if (p < a.total) {
                const uint32_t q = l + 32u - kSplitBack;   // the bit of position p - kSplitBack in s_mark
                const uint64_t two = static_cast<uint64_t>(s_mark[(q >> 5) + 1]) << 32 | s_mark[q >> 5];
                int before, ahead;
                split_reach(static_cast<uint32_t>(two >> (q & 31u)), before, ahead);
                f = split_start(a.tab, &s_txt[l + kSplitBack], before, ahead, a.rule);
            }
            const unsigned long long m = __ballot(f);
            if ((tid & 63u) == 0) {
                a.masks[p >> 6] = m;
                cnt += static_cast<uint32_t>(__popcll(m));
            }
        }
        if ((tid & 63u) == 0) s_cnt[tid >> 6] = cnt;
        __syncthreads();
        if (tid == 0) {
            unsigned long long sum = 0;
            for (uint32_t i = 0; i < kSplitLanes / 64; ++i) sum += s_cnt[i];
            a.counts[tile] = sum;
        }
        __syncthreads();   // the next tile is staged over this one
    }
}

__global__ __launch_bounds__(kSplitLanes) void split_scatter_kernel(const SplitArgs a) {
    __shared__ uint32_t s_pre[kSplitTileWords];   // the set bits of the tile's mask words in front of word j
    const uint32_t tid = threadIdx.x;
    const unsigned long long n_words = *a.n_words;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        if (tid == 0) {
            uint32_t run = 0;
            for (uint32_t j = 0; j < kSplitTileWords; ++j) {
                s_pre[j] = run;
                run += static_cast<uint32_t>(__popcll(a.masks[tile * kSplitTileWords + j]));
            }
        }
        __syncthreads();
        const unsigned long long first = a.counts[tile];
        for (uint32_t it = 0; it < kSplitTile / kSplitLanes; ++it) {
            const uint32_t l = it * kSplitLanes + tid;
            const unsigned long long m = a.masks[tile * kSplitTileWords + (l >> 6)];
            const uint32_t bit = l & 63u;
            if ((m >> bit) & 1ull) {
                const unsigned long long rank = first + s_pre[l >> 6] + static_cast<uint32_t>(__popcll(m & ((1ull << bit) - 1ull)));
                if (rank < n_words) a.word_offsets[rank] = a.base + tile * kSplitTile + l;
            }
        }
        __syncthreads();
    }
}

// ---- DAAC_SPLIT_CL100K / DAAC_SPLIT_LLAMA3: sum, carry, flags
struct SplitTileLds {
    uint8_t txt[kSplitTile + 32];             // entry kSplitBack + l: the byte of the tile's position l
    uint32_t mark[kSplitMarkWords + 2];       // entry 1 + j: the tile's mark word j
    uint64_t raw[7][kSplitTileWords];         // the ballots of the predicate bits kPredU .. kPredO, the mark and the mark one on
    SplitPlanes pl[kSplitTileWords];
    uint32_t wsum[kSplitTileWords];           // what each word does to the states
    uint32_t cf[kSplitTileWords];             // the forward states in front of each word
    uint32_t cb[kSplitTileWords];             // the backward states behind each word
    uint32_t cnt[kSplitLanes / 64];
};

// before and ahead of the tile's position l, and the marks of the position (bit 0) and of the one behind it (bit 1)
static __device__ __forceinline__ uint32_t split_tile_reach(const SplitTileLds &s, uint32_t l, int &before, int &ahead) {
    const uint32_t q = l + 32u - kSplitBack;   // the bit of position p - kSplitBack in s.mark
    const uint64_t two = static_cast<uint64_t>(s.mark[(q >> 5) + 1]) << 32 | s.mark[q >> 5];
    const uint32_t win = static_cast<uint32_t>(two >> (q & 31u));
    split_reach(win, before, ahead);
    return (win >> kSplitBack) & 3u;
}

// Stages a tile and builds the masks and the functions of its words.  Ends behind a barrier.
static __device__ __forceinline__ void split_tile_planes(const SplitArgs &a, uint64_t tile, SplitTileLds &s) {
    const uint32_t tid = threadIdx.x;
    const uint64_t n_mark = a.tiles * kSplitMarkWords + 1;
    const uint64_t base = tile * kSplitTile;
    for (uint32_t i = tid; i < kSplitTile + kSplitBack + kSplitAhead - 1; i += kSplitLanes) {
        const uint64_t p = base + i;   // the position + kSplitBack
        s.txt[i] = p >= static_cast<uint64_t>(kSplitBack) && p - kSplitBack < a.total ? a.text[p - kSplitBack] : static_cast<uint8_t>(0);
    }
    for (uint32_t i = tid; i < kSplitMarkWords + 2; i += kSplitLanes) {
        const uint64_t w = tile * kSplitMarkWords + i;   // the word + 1
        s.mark[i] = w >= 1 && w - 1 < n_mark ? a.marks[w - 1] : 0u;
    }
    __syncthreads();
    for (uint32_t it = 0; it < kSplitTile / kSplitLanes; ++it) {
        const uint32_t l = it * kSplitLanes + tid;
        uint32_t bits = 0, mk = 0;
        if (base + l < a.total) {
            int before, ahead;
            mk = split_tile_reach(s, l, before, ahead);
            bits = split_pred(a.tab, &s.txt[l + kSplitBack], before, ahead);
        }
        // one ballot at a time, each to LDS by the wave's first lane
        const uint32_t all = bits | mk << 5, w = l >> 6;
        for (uint32_t b = 0; b < 7; ++b) {
            const uint64_t m = __ballot((all >> b) & 1u);
            if ((tid & 63u) == 0) s.raw[b][w] = m;
        }
    }
    __syncthreads();
    if (tid < kSplitTileWords) {
        const SplitPlanes p = split_planes(s.raw[0][tid], s.raw[1][tid], s.raw[2][tid], s.raw[3][tid], s.raw[4][tid], s.raw[5][tid], s.raw[6][tid]);
        s.pl[tid] = p;
        s.wsum[tid] = split_word_sum(p);
    }
    __syncthreads();
}

// A workgroup takes one tile (the grid's second dimension counts on behind kSplitMaxBlocks tiles): with no loop over tiles nothing of a
// tile's work is kept in registers for the next one.
static __device__ __forceinline__ uint64_t split_tile_of_block() { return static_cast<uint64_t>(blockIdx.y) * gridDim.x + blockIdx.x; }

__global__ __launch_bounds__(kSplitLanes) void split_sum_kernel(const SplitArgs a) {
    __shared__ SplitTileLds s;
    const uint64_t tile = split_tile_of_block();
    if (tile >= a.tiles) return;
    split_tile_planes(a, tile, s);
    if (threadIdx.x == 0) a.tile_sum[tile] = split_span_sum(s.wsum, 0, kSplitTileWords);
}

// One workgroup: lane t owns the tiles [t * chunk, (t + 1) * chunk).
__global__ __launch_bounds__(kSplitCarryLanes) void split_carry_kernel(const SplitArgs a) {
    __shared__ uint32_t s_sum[kSplitCarryLanes], s_f[kSplitCarryLanes], s_b[kSplitCarryLanes];
    const uint32_t tid = threadIdx.x;
    const uint64_t chunk = (a.tiles + kSplitCarryLanes - 1) / kSplitCarryLanes;
    const uint64_t begin = tid * chunk < a.tiles ? tid * chunk : a.tiles, end = begin + chunk < a.tiles ? begin + chunk : a.tiles;
    s_sum[tid] = split_span_sum(a.tile_sum, begin, end);
    __syncthreads();
    if (tid == 0) split_span_carries(s_sum, 0, kSplitCarryLanes, 0u, 0u, s_f, s_b);
    __syncthreads();
    split_span_carries(a.tile_sum, begin, end, s_f[tid], s_b[tid], a.carry_f, a.carry_b);
}

__global__ __launch_bounds__(kSplitLanes) void split_flag_scanned_kernel(const SplitArgs a) {
    __shared__ SplitTileLds s;
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = split_tile_of_block();
    if (tile >= a.tiles) return;
    const uint64_t base = tile * kSplitTile;
    split_tile_planes(a, tile, s);
    if (tid == 0) split_span_carries(s.wsum, 0, kSplitTileWords, a.carry_f[tile], a.carry_b[tile], s.cf, s.cb);
    __syncthreads();
    uint32_t cnt = 0;
    for (uint32_t it = 0; it < kSplitTile / kSplitLanes; ++it) {
        const uint32_t l = it * kSplitLanes + tid;
        const uint64_t p = base + l;
        bool f = false;
        if (p < a.total) {
            int before, ahead;
            (void)split_tile_reach(s, l, before, ahead);
            const SplitScan sc = split_scan_at(s.pl[l >> 6], l & 63u, s.cf[l >> 6], s.cb[l >> 6]);
            f = split_start_scanned(a.tab, &s.txt[l + kSplitBack], before, ahead, a.rule, sc);
        }
        const unsigned long long m = __ballot(f);
        if ((tid & 63u) == 0) {
            a.masks[p >> 6] = m;
            cnt += static_cast<uint32_t>(__popcll(m));
        }
    }
    if ((tid & 63u) == 0) s.cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long sum = 0;
        for (uint32_t i = 0; i < kSplitLanes / 64; ++i) sum += s.cnt[i];
        a.counts[tile] = sum;
    }
}

// ---- DAAC_SPLIT_O200K: sum, carry, flags
constexpr uint32_t kSplitIters = kSplitTile / kSplitLanes;   // positions of a lane
struct O200kTileLds {
    uint8_t txt[kSplitTile + 32];             // entry kSplitBack + l: the byte of the tile's position l
    uint32_t mark[kSplitMarkWords + 2];       // entry 1 + j: the tile's mark word j
    unsigned long long wmap[kSplitTileWords]; // what each word does to the forward state
    uint32_t wback[kSplitTileWords];          // what each word does to (f, g)
    uint32_t cf[kSplitTileWords];             // the forward state in front of each word
    uint32_t cb[kSplitTileWords];             // the backward bits behind each word
    uint32_t cnt[kSplitLanes / 64];
};

// What a lane keeps of its positions between the scan and the decision: the info, the map of the wave's positions in front of it
// and the (f, g) function of the wave's positions from it on.
struct O200kLane {
    uint32_t info[kSplitIters];
    uint64_t ex[kSplitIters];
    uint32_t back[kSplitIters];
};

// Stages a tile, takes every position's two functions and composes them inside each wave; the words' totals go to LDS.  Ends behind a
// barrier.
static __device__ __forceinline__ void o200k_tile_scan(const SplitArgs &a, uint64_t tile, O200kTileLds &s, O200kLane &r) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t n_mark = a.tiles * kSplitMarkWords + 1;
    const uint64_t base = tile * kSplitTile;
    for (uint32_t i = tid; i < kSplitTile + kSplitBack + kSplitAhead - 1; i += kSplitLanes) {
        const uint64_t p = base + i;   // the position + kSplitBack
        s.txt[i] = p >= static_cast<uint64_t>(kSplitBack) && p - kSplitBack < a.total ? a.text[p - kSplitBack] : static_cast<uint8_t>(0);
    }
    for (uint32_t i = tid; i < kSplitMarkWords + 2; i += kSplitLanes) {
        const uint64_t w = tile * kSplitMarkWords + i;   // the word + 1
        s.mark[i] = w >= 1 && w - 1 < n_mark ? a.marks[w - 1] : 0u;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t it = 0; it < kSplitIters; ++it) {
        const uint32_t l = it * kSplitLanes + tid;
        uint32_t info = 0, bk = kBackIdentity;
        uint64_t m = kO200kIdentity;
        if (base + l < a.total) {
            const uint32_t q = l + 32u - kSplitBack;   // the bit of position p - kSplitBack in s.mark
            const uint64_t two = static_cast<uint64_t>(s.mark[(q >> 5) + 1]) << 32 | s.mark[q >> 5];
            const uint32_t win = static_cast<uint32_t>(two >> (q & 31u));
            int before, ahead;
            split_reach(win, before, ahead);
            info = o200k_info(a.tab, &s.txt[l + kSplitBack], before, ahead);
            m = o200k_fwd_of(info, (win >> kSplitBack) & 1u);
            bk = o200k_back_of(info, (win >> (kSplitBack + 1)) & 1u);
        }
        for (uint32_t d = 1; d < 64; d <<= 1) {   // the wave's scans: the positions up to and including the lane's, and those from it on
            const uint64_t mo = __shfl_up(static_cast<unsigned long long>(m), d);
            const uint32_t bo = __shfl_down(bk, d);
            if (lane >= d) m = o200k_then(mo, m);
            if (lane + d < 64u) bk = o200k_back_then(bo, bk);
        }
        const uint64_t ex = __shfl_up(static_cast<unsigned long long>(m), 1u);
        r.info[it] = info;
        r.ex[it] = lane ? ex : kO200kIdentity;
        r.back[it] = bk;
        if (lane == 63u) s.wmap[l >> 6] = m;
        if (lane == 0u) s.wback[l >> 6] = bk;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kSplitLanes) void split_o200k_sum_kernel(const SplitO200kArgs g) {
    __shared__ O200kTileLds s;
    const uint64_t tile = split_tile_of_block();
    if (tile >= g.a.tiles) return;
    O200kLane r;
    o200k_tile_scan(g.a, tile, s, r);
    if (threadIdx.x == 0) g.tile_map[tile] = o200k_span_map(s.wmap, 0, kSplitTileWords);
    if (threadIdx.x == 64) g.a.tile_sum[tile] = o200k_span_back(s.wback, 0, kSplitTileWords);
}

// One workgroup: lane t owns the tiles [t * chunk, (t + 1) * chunk).
__global__ __launch_bounds__(kSplitCarryLanes) void split_o200k_carry_kernel(const SplitO200kArgs g) {
    __shared__ unsigned long long s_map[kSplitCarryLanes];
    __shared__ uint32_t s_back[kSplitCarryLanes], s_f[kSplitCarryLanes], s_b[kSplitCarryLanes];
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = g.a.tiles, chunk = (tiles + kSplitCarryLanes - 1) / kSplitCarryLanes;
    const uint64_t begin = tid * chunk < tiles ? tid * chunk : tiles, end = begin + chunk < tiles ? begin + chunk : tiles;
    s_map[tid] = o200k_span_map(g.tile_map, begin, end);
    s_back[tid] = o200k_span_back(g.a.tile_sum, begin, end);
    __syncthreads();
    if (tid == 0) o200k_span_carries(s_map, s_back, 0, kSplitCarryLanes, kQNone, 0u, s_f, s_b);
    __syncthreads();
    o200k_span_carries(g.tile_map, g.a.tile_sum, begin, end, s_f[tid], s_b[tid], g.a.carry_f, g.a.carry_b);
}

__global__ __launch_bounds__(kSplitLanes) void split_o200k_flag_kernel(const SplitO200kArgs g) {
    __shared__ O200kTileLds s;
    const SplitArgs &a = g.a;
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = split_tile_of_block();
    if (tile >= a.tiles) return;
    const uint64_t base = tile * kSplitTile;
    O200kLane r;
    o200k_tile_scan(a, tile, s, r);
    if (tid == 0) o200k_span_carries(s.wmap, s.wback, 0, kSplitTileWords, a.carry_f[tile], a.carry_b[tile], s.cf, s.cb);
    __syncthreads();
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t it = 0; it < kSplitIters; ++it) {
        const uint32_t l = it * kSplitLanes + tid;
        const uint64_t p = base + l;
        bool f = false;
        if (p < a.total) {
            int before, ahead;
            const uint32_t q = l + 32u - kSplitBack;
            const uint64_t two = static_cast<uint64_t>(s.mark[(q >> 5) + 1]) << 32 | s.mark[q >> 5];
            split_reach(static_cast<uint32_t>(two >> (q & 31u)), before, ahead);
            f = o200k_start(a.tab, &s.txt[l + kSplitBack], before, ahead, r.info[it], o200k_apply(r.ex[it], s.cf[l >> 6]), o200k_back_apply(r.back[it], s.cb[l >> 6]));
        }
        const unsigned long long m = __ballot(f);
        if ((tid & 63u) == 0) {
            a.masks[p >> 6] = m;
            cnt += static_cast<uint32_t>(__popcll(m));
        }
    }
    if ((tid & 63u) == 0) s.cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned long long sum = 0;
        for (uint32_t i = 0; i < kSplitLanes / 64; ++i) sum += s.cnt[i];
        a.counts[tile] = sum;
    }
}

// doc_words[d] = the word starts in front of document d's first position; the lane behind the last document closes both lists
__global__ __launch_bounds__(256) void split_docs_kernel(const SplitArgs a) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const unsigned long long n_words = *a.n_words;
    for (uint64_t d = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d <= a.n_docs; d += stride) {
        const uint64_t off = a.doc_off[d];
        const uint64_t p = off < a.base ? 0 : off - a.base;
        unsigned long long rank = n_words;
        if (p < a.total) {
            const uint64_t tile = p / kSplitTile;
            const uint32_t l = static_cast<uint32_t>(p % kSplitTile);
            rank = a.counts[tile];
            for (uint32_t j = 0; j < (l >> 6); ++j) rank += static_cast<uint32_t>(__popcll(a.masks[tile * kSplitTileWords + j]));
            rank += static_cast<uint32_t>(__popcll(a.masks[tile * kSplitTileWords + (l >> 6)] & ((1ull << (l & 63u)) - 1ull)));
        }
        a.doc_words[d] = rank;
        if (d == a.n_docs) a.word_offsets[n_words] = a.base + a.total;
    }
}

__global__ __launch_bounds__(256) void offsets_compose_kernel(const unsigned long long *inner, const unsigned long long *outer, uint64_t n, unsigned long long *out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = inner[outer[i]];
}

__global__ __launch_bounds__(256) void spans_rebase_kernel(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *word_offsets,
                                                           const unsigned long long *doc_words, const unsigned long long *doc_off, uint64_t n_words, uint64_t n_docs) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < n_words; w += stride) {
        uint64_t lo = 0, hi = n_docs;   // the last document d with doc_words[d] <= w: the word's (empty documents share an entry)
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (doc_words[mid] <= w) lo = mid; else hi = mid;
        }
        const unsigned long long delta = word_offsets[w] - doc_off[lo];
        const unsigned long long e = tok_offsets[w + 1];
        for (unsigned long long t = tok_offsets[w]; t < e; ++t) {
            spans[2 * t] += delta;
            spans[2 * t + 1] += delta;
        }
    }
}

// flags[w] = whether word w is whitespace: one lane per word
__global__ __launch_bounds__(256) void split_words_space_kernel(const SplitTable tab, const uint8_t *text, const unsigned long long *word_offsets, uint64_t n_words,
                                                                uint64_t lo, uint64_t hi, uint8_t *flags) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < n_words; w += stride) {
        const uint64_t b = word_offsets[w], e = word_offsets[w + 1];
        flags[w] = b >= lo && e <= hi ? split_word_space(tab, text, b, e) : static_cast<uint8_t>(0);   // (a word outside the text: never, from split_batch)
    }
}

__global__ __launch_bounds__(256) void split_words_space_o200k_kernel(const SplitTable tab, const uint8_t *text, const unsigned long long *word_offsets, uint64_t n_words,
                                                                      uint64_t lo, uint64_t hi, uint8_t *flags) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < n_words; w += stride) {
        const uint64_t b = word_offsets[w], e = word_offsets[w + 1];
        flags[w] = b >= lo && e <= hi ? o200k_word_space(tab, text, b, e) : static_cast<uint8_t>(0);
    }
}

static uint32_t split_grid(uint64_t items, uint32_t per_block, uint32_t cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return static_cast<uint32_t>(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_split_marks(const SplitArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(split_mark_kernel, dim3(split_grid(a.n_docs + 1, 256, 4096)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_split_flags(const SplitArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(split_flag_kernel, dim3(split_grid(a.tiles, 1, kSplitMaxBlocks)), dim3(kSplitLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_split_flags_scanned(const SplitArgs &a, hipStream_t stream) {
    const uint32_t gx = split_grid(a.tiles, 1, kSplitMaxBlocks), gy = static_cast<uint32_t>((a.tiles + gx - 1) / gx);   // a workgroup per tile
    if (gy > 65535u) return hipErrorInvalidValue;   // (2^36 tiles: never)
    hipLaunchKernelGGL(split_sum_kernel, dim3(gx, gy), dim3(kSplitLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(split_carry_kernel, dim3(1), dim3(kSplitCarryLanes), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(split_flag_scanned_kernel, dim3(gx, gy), dim3(kSplitLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_split_flags_o200k(const SplitO200kArgs &g, hipStream_t stream) {
    const uint32_t gx = split_grid(g.a.tiles, 1, kSplitMaxBlocks), gy = static_cast<uint32_t>((g.a.tiles + gx - 1) / gx);   // a workgroup per tile
    if (gy > 65535u) return hipErrorInvalidValue;   // (2^36 tiles: never)
    hipLaunchKernelGGL(split_o200k_sum_kernel, dim3(gx, gy), dim3(kSplitLanes), 0, stream, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(split_o200k_carry_kernel, dim3(1), dim3(kSplitCarryLanes), 0, stream, g);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(split_o200k_flag_kernel, dim3(gx, gy), dim3(kSplitLanes), 0, stream, g);
    return hipGetLastError();
}

hipError_t launch_split_scatter(const SplitArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(split_scatter_kernel, dim3(split_grid(a.tiles, 1, kSplitMaxBlocks)), dim3(kSplitLanes), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(split_docs_kernel, dim3(split_grid(a.n_docs + 1, 256, 4096)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_offsets_compose(const unsigned long long *inner, const unsigned long long *outer, uint64_t n, unsigned long long *out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(offsets_compose_kernel, dim3(split_grid(n, 256, 4096)), dim3(256), 0, stream, inner, outer, n, out);
    return hipGetLastError();
}

hipError_t launch_spans_rebase(unsigned long long *spans, const unsigned long long *tok_offsets, const unsigned long long *word_offsets,
                               const unsigned long long *doc_words, const unsigned long long *doc_off, uint64_t n_words, uint64_t n_docs, hipStream_t stream) {
    if (n_words == 0 || n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(spans_rebase_kernel, dim3(split_grid(n_words, 256, 4096)), dim3(256), 0, stream, spans, tok_offsets, word_offsets, doc_words, doc_off,
                       n_words, n_docs);
    return hipGetLastError();
}

hipError_t launch_split_words_space(const SplitTable &tab, const uint8_t *text, const unsigned long long *word_offsets, uint64_t n_words, uint64_t lo, uint64_t hi,
                                    uint8_t *flags, hipStream_t stream, bool o200k) {
    if (n_words == 0) return hipSuccess;
    if (o200k) {
        hipLaunchKernelGGL(split_words_space_o200k_kernel, dim3(split_grid(n_words, 256, 4096)), dim3(256), 0, stream, tab, text, word_offsets, n_words, lo, hi, flags);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(split_words_space_kernel, dim3(split_grid(n_words, 256, 4096)), dim3(256), 0, stream, tab, text, word_offsets, n_words, lo, hi, flags);
    return hipGetLastError();
}
#endif

}  // namespace daac
