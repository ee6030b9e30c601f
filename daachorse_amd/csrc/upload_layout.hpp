// The layout layer of the upload: what lies between the table builders (repack.hpp, gram*.hpp, pfx.hpp, char_tables.hpp) and the kernels.
// One function per table set turns the builder's vectors into the arrays a kernel reads (LDS addresses in place of ids, rank blobs, hash
// tables, packed records), works out the LDS offsets and padded sizes of its *Dev struct and applies the gates behind the *_ok flags.
//
// Plain C++: nothing here calls the HIP runtime or reads an option.  An array leaves through a SINK — any type with
//      template <class T> daac_status put(const std::vector<T> &v, const T *&out);
// which takes the vector and gives back the pointer the *Dev field gets.  The device sink is DeviceTables::put (api_internal.hpp: padded
// allocation, zero fill, copy); tests/native/upload_layout_check.cpp records sizes and hashes instead, on the CPU.  The options a layout
// depends on come in as UploadOptions, which upload_locked (api_upload.hip) fills once.
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "charwise.hpp"
#include "device_tables.hpp"
#include "gram.hpp"
#include "gram2.hpp"
#include "gram2w.hpp"
#include "gram4.hpp"
#include "pfx.hpp"
#include "pma.hpp"
#include "repack.hpp"

namespace daac {

constexpr uint32_t kWorkgroupLds = 160u << 10;   // the 160 KB of LDS a workgroup can have on gfx950
constexpr uint32_t kHitRingEntries = 128, kWavesPerWorkgroup = 16;
constexpr uint32_t kHitRingBytes = kWavesPerWorkgroup * kHitRingEntries * 8u;   // one ring of 8-byte entries per wave of a 1024-thread workgroup
inline uint32_t pad16(size_t x) { return static_cast<uint32_t>((x + 15) & ~size_t(15)); }

// The options read when a handle's tables are laid out, by their names in DAAC_OPTIONS (api_internal.hpp).
struct UploadOptions {
    int64_t lds_budget, dense_depth, rows_share_pct;   // TIERED
    int64_t gram_lds_budget, gram_rank_in_lds;         // GRAM: the tables' LDS (v1, v2, wide); v1's rank directory in LDS (-1: decide)
    int64_t gram4_mph, gram2_rfull, gram2_dpp;
    int64_t left3, pfx;
    int64_t char_map_lds, char_row_lds;
};

// What an upload computes: every engine's kernel arguments and whether the engine serves the handle.  (What a handle's device state keeps
// at run time beside it — counters, the kept workspace, the allocations — is DeviceTables', api_internal.hpp.)
struct EngineTables {
    bool tier_ok = false;
    TierDev tier{};
    DArrayDev da{};
    TierTables tier_host_meta;  // sizes only (vectors cleared after upload)
    bool gram_ok = false;
    GramDev gram{};
    bool gram2_ok = false;     // second table set (gram2.hpp)
    Gram2Dev gram2{};
    bool gram4_ok = false;     // `.count()` tables of round 5 (gram4.hpp), derived from the second table set
    Gram4Dev gram4{};
    bool gramw_ok = false;     // wide alphabets (gram2w.hpp)
    bool pfx_ok = false;       // any byte alphabet, `.count()` (pfx.hpp)
    uint32_t n_distinct_bytes = 0;  // distinct pattern bytes (known when the PFX builder ran)
    PfxDev pfx{};
    Gram2WDev gramw{};
    Gram2EmitDev emit{};
    bool emit3_ok = false;     // ... with detection done once (emit3_kernels.hip)
    Gram3Lds emit3_lds{};
    bool emit3_has_len1 = false;   // some pattern is a single byte
    const uint32_t *pfx_probe_word = nullptr;   // device word the probe kernel leaves its count in
    bool find3_ok = false;         // find_iter's count / checksum without a state chain (find3_kernels.hip): K = 3, no pattern beyond 19 bytes
    Find3Dev find3{};
    Find3Dev find3v{};             // the same tables with the patterns' VALUES (the emitter's V1 / V2 / V3 rank structure): the selection's tuple list
    bool left3_ok = false;         // a leftmost handle whose patterns, as a Standard automaton, got the emitter's and find3's tables: left3_kernels.hip serves leftmost_find_iter
    bool pfx_emit_ok = false;      // PFX tuples: pfx_emit_kernel + EXPAND over the raw haystack (no pattern registered twice)
    Gram2EmitDev pfx_emit{};       // what that EXPAND needs: V1 by byte + the 256 flag bytes (v1, v1_bytes = 1280), K = 1
    CharDev chr{};  // charwise automata only
};

namespace layout {

#define LAYOUT_TRY(expr)                             \
    do {                                             \
        const daac_status st_ = (expr);              \
        if (st_ != DAAC_OK) return st_;              \
    } while (0)

// put() for a field whose element type is the device's name for the host's record (uint4 for U32x4, uint2 for OutSum, ...)
template <class Sink, class T, class D>
daac_status put_as(Sink &sink, const std::vector<T> &v, const D *&out) {
    static_assert(sizeof(T) == sizeof(D), "the same record under two names");
    const T *p = nullptr;
    LAYOUT_TRY(sink.put(v, p));
    out = reinterpret_cast<const D *>(p);
    return DAAC_OK;
}

// hit records with the first child beside them: one request instead of a dependent second one
inline std::vector<U32x4> zip_first_child(const std::vector<U32x2> &hit, const std::vector<uint32_t> &first) {
    std::vector<U32x4> out(hit.size());
    for (size_t i = 0; i < hit.size(); ++i) out[i] = U32x4{hit[i].x, hit[i].y, first[i], 0u};
    return out;
}

// ----------------------------------------------------------------------------------- outputs, shared by all engines
struct OutputsDev {
    const uint32_t *outputs = nullptr;   // n_outputs x {value, length, parent}
    const uint32_t *ohash = nullptr;     // n_outputs x h32 of the record's own match
};
template <class Sink>
daac_status outputs(const std::vector<OutputRec> &outs, OutputsDev &o, Sink &sink) {
    std::vector<uint32_t> flat(outs.size() * 3);
    for (size_t i = 0; i < outs.size(); ++i) {
        flat[3 * i] = outs[i].value; flat[3 * i + 1] = outs[i].length; flat[3 * i + 2] = outs[i].parent;
    }
    LAYOUT_TRY(sink.put(flat, o.outputs));
    std::vector<uint32_t> oh(outs.size());
    for (size_t i = 0; i < outs.size(); ++i) oh[i] = match_hash32(outs[i].value, outs[i].length);
    return sink.put(oh, o.ohash);
}

// ----------------------------------------------------------------------------------- charwise
// The chain walkers' child filters (device_tables.hpp, CharDev::wstates): a slot t >= 2 whose CHECK names a state p other than DEAD is p's
// child on code t ^ base(p) (vacant slots: CHECK = DEAD, reference src/charwise.rs:1103-1112)
inline std::vector<uint32_t> char_child_filters(const CharTables &ct, uint32_t alphabet_size, uint32_t fbits) {
    std::vector<uint32_t> filt(ct.states.size(), 0u);
    if (fbits == 0) return filt;
    for (size_t tt = 2; tt < ct.states.size(); ++tt) {
        const uint32_t pp = ct.states[tt].check;
        if (pp == 1u || pp >= ct.states.size() || ct.states[pp].base == 0) continue;
        const uint32_t code = static_cast<uint32_t>(tt) ^ ct.states[pp].base;
        if (code >= alphabet_size) continue;
        filt[pp] |= 1u << (code & (fbits - 1u));
    }
    return filt;
}

// ROOT's row of children for the chain walkers: a lane at ROOT (where failed walks end) then needs no memory at all.
// Staged beside the mapper when both fit 80 KB (two 1024-lane workgroups per CU) and every child packs into 8 bytes.
template <class Sink>
daac_status char_root_row(const CharTables &ct, const std::vector<uint32_t> &filt, const UploadOptions &o, CharDev &c, Sink &sink) {
    const uint32_t A = c.alphabet;
    std::vector<U32x2> row(A, U32x2{2u << 30, 0u});
    bool ok = c.map_in_lds != 0 && o.char_row_lds != 0 && A != 0;
    const CStateRec &rt = ct.states[0];
    for (uint32_t code = 0; ok && code < A; ++code) {
        if (rt.base == 0) break;
        const uint32_t child = rt.base ^ code;
        if (child >= ct.states.size() || ct.states[child].check != 0) continue;
        const CStateRec &ch = ct.states[child];
        const uint32_t fl = (c.leftmost || ct.fail_plain.empty()) ? ch.fail : ct.fail_plain[child];
        if (fl > 1u || (fl == 1u && !c.leftmost) || ch.base >= (1u << 30)) ok = false;
        row[code] = U32x2{ch.base | (fl << 30), ch.output_pos | (c.fbits ? filt[child] << c.obits : 0u)};
    }
    const uint32_t map_bytes = pad16((128u + c.table_len - c.map_lo) * 2u);
    ok = ok && map_bytes + A * 8u <= 80u * 1024u;
    c.row_in_lds = ok;
    c.root_row = nullptr;
    return ok ? put_as(sink, row, c.root_row) : DAAC_OK;
}

template <class Sink>
daac_status charwise(const HostCharPma &p, const UploadOptions &o, const OutputsDev &outs, EngineTables &e, Sink &sink) {
    CharTables ct;
    build_char_tables(p, ct);
    CharDev &c = e.chr;
    LAYOUT_TRY(put_as(sink, ct.states, c.states));
    LAYOUT_TRY(sink.put(ct.table, c.table));
    LAYOUT_TRY(put_as(sink, ct.osum, c.osum));
    c.fail_plain = nullptr;
    if (!ct.fail_plain.empty()) LAYOUT_TRY(sink.put(ct.fail_plain, c.fail_plain));
    c.outputs = outs.outputs;
    c.ohash = outs.ohash;
    c.table_len = static_cast<uint32_t>(ct.table.size());
    c.n = static_cast<uint32_t>(ct.states.size());
    c.root_flag = ct.root_flag;
    c.leftmost = !p.is_standard();
    c.alphabet = p.alphabet_size;
    // Stage [map_lo, table_len) of the mapper in LDS when that stretch is small: map_lo = the lowest start for which
    // it fits 32 KB, moved up to the first mapped code point at or above it (CJK text: the table is dense from the
    // kana up, ASCII below stays in L2).
    {
        const uint32_t cap = 16u * 1024u - 128u;  // u16 entries (128 more hold ASCII)
        uint32_t lo = c.table_len > cap ? c.table_len - cap : 0u;
        while (lo < c.table_len && ct.table[lo] == kInvalidCode) ++lo;
        c.map_lo = lo;
        uint32_t staged = 0;
        for (uint32_t i = lo; i < c.table_len; ++i) staged += ct.table[i] != kInvalidCode;
        // worth it only if most of the alphabet lives in the stretch
        c.map_in_lds = o.char_map_lds != 0 && lo < c.table_len && p.alphabet_size < 0xffffu && staged * 4u >= p.alphabet_size * 3u;
    }
    // the walkers' records: the output_pos word also carries the state's child filter (device_tables.hpp, CharDev::wstates)
    const size_t n_out = p.outputs.size();
    c.obits = n_out < (1u << 16) ? 16u : n_out < (1u << 24) ? 24u : 0u;
    c.fbits = c.obits == 16u ? 16u : c.obits == 24u ? 8u : 0u;
    const std::vector<uint32_t> filt = char_child_filters(ct, p.alphabet_size, c.fbits);
    std::vector<CStateRec> ws(ct.states);
    if (c.fbits != 0) for (size_t i = 0; i < ws.size(); ++i) ws[i].output_pos |= filt[i] << c.obits;
    LAYOUT_TRY(put_as(sink, ws, c.wstates));
    return char_root_row(ct, filt, o, c, sink);
}

// ----------------------------------------------------------------------------------- DARRAY: always available
template <class Sink>
daac_status darray(const HostPma &h, const OutputsDev &outs, EngineTables &e, Sink &sink) {
    DArrayTables da;
    build_darray_tables(h, da);
    DArrayDev &d = e.da;
    LAYOUT_TRY(put_as(sink, da.hot, d.hot));
    LAYOUT_TRY(sink.put(da.fail, d.fail));
    d.fail_plain = d.fail;
    if (!da.fail_plain.empty()) LAYOUT_TRY(sink.put(da.fail_plain, d.fail_plain));
    d.leftmost = !h.is_standard();
    LAYOUT_TRY(put_as(sink, da.root, d.root));
    LAYOUT_TRY(put_as(sink, da.osum, d.osum));
    std::vector<U32x4> rec(da.hot.size());
    for (size_t i = 0; i < da.hot.size(); ++i) rec[i] = U32x4{da.hot[i].x, da.hot[i].y, da.fail[i], da.fmap[i]};
    LAYOUT_TRY(put_as(sink, rec, d.rec));
    LAYOUT_TRY(put_as(sink, da.root_chain, d.root_chain));
    d.outputs = outs.outputs;
    d.ohash = outs.ohash;
    d.n = static_cast<uint32_t>(h.states_len());
    d.root_flag = output_pos_of(h.opos_ch(kRoot)) != 0;
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- GRAM v1, derived from the tier tables
template <class Sink>
daac_status gram1(const HostPma &h, const TierTables &tt, const UploadOptions &o, EngineTables &e, Sink &sink) {
    GramTables gt;
    // (the option bounds the tables; tables AND the hit rings of a 1024-thread workgroup have to fit the LDS a workgroup can have)
    const int64_t budget = std::min<int64_t>(o.gram_lds_budget, kWorkgroupLds - kHitRingBytes);
    if (!(tt.N < (1u << 27) && budget > 0 && build_gram_tables(h, tt, static_cast<uint32_t>(budget), gt))) return DAAC_OK;
    GramDev &g = e.gram;
    std::vector<uint32_t> cls32(gt.cls.begin(), gt.cls.end());
    LAYOUT_TRY(sink.put(cls32, g.cls32));
    LAYOUT_TRY(sink.put(gt.cid, g.cid));
    LAYOUT_TRY(put_as(sink, gt.combo, g.combo));
    LAYOUT_TRY(sink.put(gt.bbits, g.bbits));
    LAYOUT_TRY(sink.put(gt.brank, g.brank));
    LAYOUT_TRY(sink.put(gt.bsuper, g.bsuper));
    LAYOUT_TRY(put_as(sink, gt.drec, g.drec));
    LAYOUT_TRY(put_as(sink, gt.dhit, g.dhit));
    LAYOUT_TRY(put_as(sink, zip_first_child(gt.dhit, gt.cfirst), g.dhit4));
    LAYOUT_TRY(sink.put(gt.cfirst, g.cfirst));
    g.has_short = gt.has_short;
    // LDS layout: [classes as u32 x 256][B bitmap][CID][COMBO][rank directory][hit stacks]; the first two sit at
    // fixed offsets so that the kernel addresses them with immediates
    g.off_bbits = 1024;
    g.off_cid = g.off_bbits + pad16(gt.bbits.size() * 4);
    g.off_combo = g.off_cid + (gt.has_short ? pad16(gt.cid.size() * 2) : 0u);   // not staged when unused
    g.off_brank = g.off_combo + (gt.has_short ? pad16(gt.combo.size() * 8) : 0u);
    // Without the rank directory two workgroups may fit one CU (<= 80 KB each); worth it when
    // the level is small, i.e. B hits are rare whatever the text.
    g.rank_in_lds = !(g.off_brank + 16u * 1024u <= 80u * 1024u && gt.dhit.size() <= 8192);
    if (o.gram_rank_in_lds >= 0) g.rank_in_lds = o.gram_rank_in_lds != 0;
    if (g.rank_in_lds) {
        g.off_bsuper = g.off_brank + pad16(gt.brank.size());
        g.off_scratch = g.off_bsuper + pad16(gt.bsuper.size() * 4);
    } else {
        g.off_bsuper = g.off_brank;
        g.off_scratch = g.off_brank;
    }
    g.lds_bytes = std::max<uint32_t>(g.off_scratch + kHitRingBytes, 1024u);
    g.K = gt.K; g.C = gt.C; g.CC = gt.C * gt.C; g.CCC = gt.C * gt.C * gt.C;
    g.level_start = gt.level_start;
    g.unused_byte = gt.unused_byte;
    g.n_deep = static_cast<uint32_t>(gt.dhit.size());
    e.gram_ok = g.lds_bytes <= kWorkgroupLds;
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- TIERED (and GRAM v1 where it was built)
template <class Sink>
daac_status tiered(const HostPma &h, const UploadOptions &o, const OutputsDev &outs, EngineTables &e, Sink &sink) {
    RepackOptions ro;
    ro.lds_budget = static_cast<uint32_t>(o.lds_budget);
    ro.dense_depth = static_cast<int>(o.dense_depth);
    ro.rows_share_pct = static_cast<uint32_t>(o.rows_share_pct);
    TierTables tt;
    if (!build_tier_tables(h, ro, tt)) return DAAC_OK;
    TierDev &d = e.tier;
    if (tt.row32) { const uint32_t *r32; LAYOUT_TRY(sink.put(tt.rows32, r32)); d.rows = r32; }
    else { const uint16_t *r16; LAYOUT_TRY(sink.put(tt.rows16, r16)); d.rows = r16; }
    LAYOUT_TRY(sink.put(tt.bcmap, d.bcmap));
    LAYOUT_TRY(sink.put(tt.bfail, d.bfail));
    LAYOUT_TRY(put_as(sink, tt.ssum, d.ssum));
    LAYOUT_TRY(sink.put(tt.cls, d.cls));
    LAYOUT_TRY(put_as(sink, tt.grec, d.grec));
    LAYOUT_TRY(sink.put(tt.sopos, d.sopos));
    d.outputs = outs.outputs;
    d.ohash = outs.ohash;
    d.C = tt.C; d.NA = tt.NA; d.NB = tt.NB; d.N = tt.N;
    d.off_bcmap = pad16(tt.NA * tt.C * (tt.row32 ? 4u : 2u));
    d.off_bfail = d.off_bcmap + pad16((tt.NB - tt.NA) * 4u);
    d.off_ssum = d.off_bfail + pad16((tt.NB - tt.NA) * 4u);
    d.off_cls = d.off_ssum + pad16(tt.NA * 8u);
    d.lds_bytes = std::max<uint32_t>(d.off_cls + 256u, 1024u);
    d.row32 = tt.row32;
    d.root_flag = tt.root_flag;
    e.tier_ok = true;
    LAYOUT_TRY(gram1(h, tt, o, e, sink));
    // keep the sizes for daac_pma_info
    tt.rows16.clear(); tt.rows32.clear(); tt.bcmap.clear(); tt.bfail.clear(); tt.grec.clear(); tt.ssum.clear(); tt.sopos.clear(); tt.old_of_new.clear();
    e.tier_host_meta = tt;
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- the leftmost shadow
// The patterns a bytewise automaton of either kind was built from, read back from its trie (goto edges of the double array, bytewise.rs:1070-1077)
// with their values: a state's own pattern is the output as long as the state is deep.  (LeftmostFirst: the builder never inserted what lies
// below an earlier-registered pattern, nfa_builder.rs:60-66 — what is read back is what can be reported.)  false: not a tree / "" / too large.
inline bool recover_patterns(const HostPma &p, std::vector<uint8_t> &blob, std::vector<uint64_t> &offs, std::vector<uint32_t> &vals) {
    const uint32_t n = static_cast<uint32_t>(p.states_len());
    if (n == 0 || output_pos_of(p.opos_ch(kRoot)) != 0) return false;
    constexpr uint32_t kNone = 0xffffffffu;
    std::vector<uint32_t> depth(n, kNone), parent(n, kNone), order{kRoot};
    std::vector<uint8_t> label(n, 0);
    depth[kRoot] = 0;
    for (size_t qi = 0; qi < order.size(); ++qi) {
        const uint32_t s = order[qi], base = p.base(s);
        if (base == 0) continue;
        for (uint32_t c = 0; c < 256; ++c) {
            const uint32_t t = base ^ c;
            if (t >= n || t == kRoot || t == kDead || check_of(p.opos_ch(t)) != c) continue;
            if (depth[t] != kNone) return false;
            depth[t] = depth[s] + 1; parent[t] = s; label[t] = static_cast<uint8_t>(c);
            order.push_back(t);
        }
    }
    blob.clear(); offs.assign(1, 0); vals.clear();
    std::vector<uint8_t> tmp;
    for (const uint32_t s : order) {
        if (s == kRoot) continue;
        uint32_t op = output_pos_of(p.opos_ch(s));
        bool own = false; uint32_t value = 0;
        for (int hops = 0; op != 0 && hops < 4 && op - 1 < p.outputs.size(); ++hops) {
            if (p.outputs[op - 1].length == depth[s]) { own = true; value = p.outputs[op - 1].value; break; }
            if (p.outputs[op - 1].length < depth[s]) break;
            op = p.outputs[op - 1].parent;
        }
        if (!own) continue;
        tmp.clear();
        for (uint32_t x = s; x != kRoot; x = parent[x]) tmp.push_back(label[x]);
        blob.insert(blob.end(), tmp.rbegin(), tmp.rend());
        offs.push_back(blob.size());
        vals.push_back(value);
        if (blob.size() >= (1ull << 31)) return false;
    }
    return !vals.empty();
}

// A leftmost handle gets the second table set of a Standard automaton of ITS patterns (read back from its trie) — not for any Standard scan
// (its kind forbids them) but for left3_kernels.hip, which selects leftmost_find_iter's matches among the ones the emitter's detection finds.
// The shadow is only ever used by left3, which takes dictionaries of at most 19-byte patterns over at most 29 distinct bytes: neither a
// second automaton nor its tables are built for a handle that cannot qualify.  true: `shadow` is that automaton.
inline bool leftmost_shadow(const HostPma &h, const UploadOptions &o, HostPma &shadow) {
    if (h.is_standard() || o.left3 == 0 || output_pos_of(h.opos_ch(kRoot)) != 0 || h.max_pattern_len() > 19) return false;
    std::vector<uint8_t> blob; std::vector<uint64_t> offs; std::vector<uint32_t> vals;
    if (!recover_patterns(h, blob, offs, vals)) return false;
    bool seen[256] = {false};
    uint32_t distinct = 0;
    for (uint8_t c : blob) if (!seen[c]) { seen[c] = true; ++distinct; }
    return distinct <= 29 && build_bytewise(blob.data(), offs.data(), vals.data(), vals.size(), DAAC_STANDARD, 16, shadow) == DAAC_OK;
}

// ----------------------------------------------------------------------------------- GRAM v2: built from the automaton itself
// `g2` is left for gram4() and emitter(), which derive their tables from it where e.gram2_ok.
template <class Sink>
daac_status gram2(const HostPma &h, const UploadOptions &o, Gram2Tables &g2, EngineTables &e, Sink &sink) {
    const int64_t budget = o.gram_lds_budget - static_cast<int64_t>(kHitRingBytes);
    if (!(budget > 0 && build_gram2_tables(h, static_cast<uint32_t>(budget), g2))) return DAAC_OK;
    Gram2Dev &d = e.gram2;
    LAYOUT_TRY(sink.put(g2.cls, d.cls));
    LAYOUT_TRY(sink.put(g2.m, d.m));
    if (g2.s16) {
        std::vector<uint16_t> s16(g2.sdir.begin(), g2.sdir.end());
        const uint16_t *ps;
        LAYOUT_TRY(sink.put(s16, ps));
        d.sdir = ps;
        d.s_bytes = pad16(s16.size() * 2);
    } else {
        const uint32_t *ps;
        LAYOUT_TRY(sink.put(g2.sdir, ps));
        d.sdir = ps;
        d.s_bytes = pad16(g2.sdir.size() * 4);
    }
    // CID entries are the LDS addresses of their H words (H sits at a fixed offset)
    std::vector<uint16_t> cid(g2.cid4.size());
    for (size_t i = 0; i < cid.size(); ++i) cid[i] = static_cast<uint16_t>(kGram2OffH + g2.cid4[i]);
    LAYOUT_TRY(sink.put(cid, d.cid4));
    LAYOUT_TRY(sink.put(g2.hsum, d.hsum));
    LAYOUT_TRY(put_as(sink, g2.drec, d.drec));
    LAYOUT_TRY(put_as(sink, g2.dhit, d.dhit));
    LAYOUT_TRY(put_as(sink, zip_first_child(g2.dhit, g2.cfirst), d.dhit4));
    LAYOUT_TRY(sink.put(g2.cfirst, d.cfirst));
    d.m_bytes = pad16(g2.m.size() * 4);
    d.cid_bytes = pad16(cid.size() * 2);
    d.h_bytes = pad16(g2.hsum.size() * 4);
    d.off_m_count = kGram2OffM;
    d.off_s_count = d.off_m_count + d.m_bytes;
    d.off_ring_count = d.off_s_count + d.s_bytes;
    d.lds_count = d.off_ring_count + kHitRingBytes;
    d.rfull = nullptr;
    d.rfull_ok = 0;
    if (g2.s16) {  // per-word directory for count-only launches (they have the LDS for it)
        std::vector<uint16_t> rf(g2.m.size());
        uint32_t run = 0;
        for (size_t i = 0; i < g2.m.size(); ++i) { rf[i] = static_cast<uint16_t>(run); run += static_cast<uint32_t>(__builtin_popcount(g2.m[i] & kGram2MaskBits)); }
        LAYOUT_TRY(sink.put(rf, d.rfull));
        d.rfull_bytes = pad16(rf.size() * 2);
        d.off_ring_rfull = d.off_s_count + d.rfull_bytes;
        d.lds_rfull = d.off_ring_rfull + kHitRingBytes;
        d.rfull_ok = d.lds_rfull <= static_cast<uint32_t>(o.gram_lds_budget) && o.gram2_rfull != 0;
    }
    d.off_m_exact = kGram2OffH + d.h_bytes;
    d.off_s_exact = d.off_m_exact + d.m_bytes;
    d.off_cid = d.off_s_exact + d.s_bytes;
    d.off_ring_exact = d.off_cid + d.cid_bytes;
    d.lds_exact = d.off_ring_exact + kHitRingBytes;
    d.K = g2.K; d.C = g2.C; d.s16 = g2.s16; d.unused_byte = g2.unused_byte;
    d.n_deep = static_cast<uint32_t>(g2.dhit.size());
    // the hit queue keeps the LDS address of an M word in 17 bits
    d.exact_ok = g2.exact_available && kGram2OffH + g2.hsum.size() * 4 <= 65536 && d.off_m_exact + d.m_bytes <= (1u << 17) && d.lds_exact <= kWorkgroupLds;
    d.xlane_dpp = o.gram2_dpp != 0;
    e.gram2_ok = d.off_m_count + d.m_bytes <= (1u << 17) && d.lds_count <= kWorkgroupLds;
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- gram4: tables, perfect hash, filter
// the second table set in the numbering of gram4_kernels.hip ("no pattern" last: arithmetic byte classes)
template <class Sink>
daac_status gram4(const Gram2Tables &g2, const UploadOptions &o, EngineTables &e, Sink &sink) {
    Gram4Tables g4;
    build_gram4_tables(g2, g4);
    Gram4Dev &q = e.gram4;
    q = Gram4Dev{};
    LAYOUT_TRY(sink.put(g4.cls, q.cls));
    LAYOUT_TRY(sink.put(g4.m, q.m));
    q.m_bytes = pad16(g4.m.size() * 4);
    if (g4.s16) {
        std::vector<uint16_t> s16(g4.sdir.begin(), g4.sdir.end());
        const uint16_t *ps;
        LAYOUT_TRY(sink.put(s16, ps));
        q.sdir = ps;
        q.s_bytes = pad16(s16.size() * 2);
        LAYOUT_TRY(sink.put(g4.rfull, q.rfull));
        q.rfull_bytes = pad16(g4.rfull.size() * 2);
    } else {
        const uint32_t *ps;
        LAYOUT_TRY(sink.put(g4.sdir, ps));
        q.sdir = ps;
        q.s_bytes = pad16(g4.sdir.size() * 4);
    }
    LAYOUT_TRY(put_as(sink, g4.dhit_c, q.dhit_c));
    LAYOUT_TRY(put_as(sink, g4.dhit_t, q.dhit_t));
    LAYOUT_TRY(put_as(sink, g4.drec_c, q.drec_c));
    LAYOUT_TRY(put_as(sink, g4.drec_t, q.drec_t));
    // the perfect hash over the depth-(K+1) states (gram4_mph.hpp) first: its displacement table takes the coarse directory's place in the
    // FILT workgroups' LDS — never more bytes than that — and what it is smaller goes to the Bloom array
    uint32_t front_bytes = q.s_bytes;
    if (o.gram4_mph > 0 && build_gram4_mph(g4, q.s_bytes, static_cast<uint32_t>(std::min<int64_t>(o.gram4_mph, 64)))) {
        LAYOUT_TRY(sink.put(g4.mph_disp, q.mph_disp));
        LAYOUT_TRY(put_as(sink, g4.dhit_h, q.dhit_h));
        q.mph = g4.mph;
        q.mph_bytes = front_bytes = static_cast<uint32_t>(g4.mph_disp.size());
    }
    // the filter in front of rank + gather (gram4_filter.hpp): as large as the preferred launch shape leaves room for, less a margin
    const uint32_t room = gram4_filter_room(q.m_bytes, front_bytes, g4.arith, kWorkgroupLds);
    if (room > 1024u && build_gram4_filter(g4, room - 512u)) {
        LAYOUT_TRY(sink.put(g4.bloom, q.bloom));
        q.bloom_words = static_cast<uint32_t>(g4.bloom.size());
    }
    q.K = g4.K; q.C = g4.C; q.s16 = g4.s16 ? 1u : 0u; q.arith = g4.arith ? 1u : 0u; q.lo = g4.lo; q.unused_byte = g4.unused_byte;
    q.n_deep = static_cast<uint32_t>(g4.dhit_c.size());
    e.gram4_ok = g4.available;
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- the emitter, find3 / left3
// The values of the 3-byte patterns as a rank structure for EXPAND's LDS (device_tables.hpp: v3c) and, for a dictionary of patterns of at
// most 19 bytes, find3's tables: the emitter's V1 / V2 / v3c with h32 of the pattern in place of its value (duplicates: find_iter reports
// a state's FIRST output, which is the record's own value).  `find3_built` says whether e.find3 / e.find3v were filled.
template <class Sink>
daac_status emitter_rank_tables(const Gram2Tables &g2, EngineTables &e, bool &find3_built, Sink &sink) {
    Gram2EmitDev &em = e.emit;
    find3_built = false;
    em.v3c = nullptr; em.v3c_bytes = em.v3c_dir = em.v3c_val = 0;
    if (g2.K != 3) return DAAC_OK;
    const uint32_t n3 = static_cast<uint32_t>(g2.v3.size()), nw = (n3 + 31) / 32;
    std::vector<uint32_t> bm(nw, 0), vals;
    std::vector<uint16_t> dir(nw + (nw & 1), 0);
    for (uint32_t i = 0; i < n3; ++i) {
        if ((i & 31) == 0) dir[i >> 5] = static_cast<uint16_t>(vals.size());
        if ((g2.me[i] >> 31) & 1u) { bm[i >> 5] |= 1u << (i & 31); vals.push_back(g2.v3[i]); }
    }
    if (vals.size() >= 65536) return DAAC_OK;
    std::vector<uint32_t> blob(bm);
    em.v3c_dir = static_cast<uint32_t>(blob.size() * 4);
    for (size_t i = 0; i < dir.size(); i += 2) blob.push_back(dir[i] | (static_cast<uint32_t>(dir[i + 1]) << 16));
    em.v3c_val = static_cast<uint32_t>(blob.size() * 4);
    blob.insert(blob.end(), vals.begin(), vals.end());
    while (blob.size() & 3) blob.push_back(0);
    em.v3c_bytes = static_cast<uint32_t>(blob.size() * 4);
    LAYOUT_TRY(sink.put(blob, em.v3c));
    if (g2.max_len > 19) return DAAC_OK;
    std::vector<uint32_t> h1(g2.v1.size()), h2(g2.v2.size()), hb(blob);
    for (size_t i = 0; i < h1.size(); ++i) h1[i] = match_hash32(g2.v1[i], 1);
    for (size_t i = 0; i < h2.size(); ++i) h2[i] = match_hash32(g2.v2[i], 2);
    for (size_t i = 0; i < vals.size(); ++i) hb[em.v3c_val / 4 + i] = match_hash32(vals[i], 3);
    h1.resize(em.v1_bytes / 4, 0);
    h2.resize(em.v2_bytes / 4, 0);
    Find3Dev &f = e.find3;
    LAYOUT_TRY(sink.put(h1, f.h1));
    LAYOUT_TRY(sink.put(h2, f.h2));
    LAYOUT_TRY(sink.put(hb, f.h3c));
    f.h1_bytes = em.v1_bytes; f.h2_bytes = em.v2_bytes; f.h3c_bytes = em.v3c_bytes; f.h3c_dir = em.v3c_dir; f.h3c_val = em.v3c_val; f.C = g2.C;
    e.find3v = f;
    e.find3v.h1 = em.v1; e.find3v.h2 = em.v2; e.find3v.h3c = em.v3c;
    find3_built = true;
    return DAAC_OK;
}

// Called where e.gram2_ok and g2.emit_available.  `shadow`: g2 is the shadow automaton's of a leftmost handle — the selection then serves
// leftmost_find_iter (left3) and nothing Standard (never asked of such a handle; said explicitly all the same).
template <class Sink>
daac_status emitter(const Gram2Tables &g2, bool shadow, EngineTables &e, Sink &sink) {
    const Gram2Dev &d = e.gram2;
    Gram2EmitDev &em = e.emit;
    em.cls = d.cls;
    em.sdir = d.sdir;
    em.cfirst = d.cfirst;
    LAYOUT_TRY(sink.put(g2.me, em.me));
    LAYOUT_TRY(sink.put(g2.v1, em.v1));
    LAYOUT_TRY(sink.put(g2.v2, em.v2));
    LAYOUT_TRY(sink.put(g2.v3, em.v3));
    LAYOUT_TRY(put_as(sink, g2.erec, em.erec));
    LAYOUT_TRY(put_as(sink, g2.ehit, em.ehit));
    std::vector<U32x4> h4v = zip_first_child(g2.ehit, g2.cfirst);
    for (size_t i = 0; i < h4v.size(); ++i) h4v[i].w = g2.ecopies[i] << 24;
    LAYOUT_TRY(put_as(sink, h4v, em.ehit4));
    LAYOUT_TRY(sink.put(g2.dupo, em.dupo));
    LAYOUT_TRY(sink.put(g2.dupv, em.dupv));
    em.level_start = g2.level_start;
    em.m_bytes = d.m_bytes; em.s_bytes = d.s_bytes;
    em.v1_bytes = pad16(g2.v1.size() * 4); em.v2_bytes = pad16(g2.v2.size() * 4);
    em.off_s = kGram2OffM + em.m_bytes;
    em.off_v1 = em.off_s + em.s_bytes;
    em.off_v2 = em.off_v1 + em.v1_bytes;
    em.off_ring = em.off_v2 + em.v2_bytes;
    em.off_wave = em.off_ring + kHitRingBytes;
    em.K = g2.K; em.C = g2.C; em.s16 = g2.s16; em.unused_byte = g2.unused_byte;
    bool find3_built = false;
    LAYOUT_TRY(emitter_rank_tables(g2, e, find3_built, sink));
    for (uint32_t w : g2.me) e.emit3_has_len1 = e.emit3_has_len1 || ((w >> 29) & 1u) != 0;
    // The gates, each decided once.  DETECT and EXPAND fit: DETECT as a 16-wave workgroup when the tables leave room for the text slots,
    // else 8 waves; EXPAND's two launch shapes; a staged tuple keeps its length in 22 bits.
    const bool plan_ok = emit3_plan(em, 16, kWorkgroupLds, e.emit3_lds) || emit3_plan(em, 8, kWorkgroupLds, e.emit3_lds);
    const bool fits = plan_ok && emit3_expand_lds_bytes(em, 4, false, false) <= 64u * 1024u && emit3_expand_lds_bytes(em, 8, true, false) <= 80u * 1024u &&
                      g2.max_len < (1u << 22);
    // The selection over DETECT's stream (find_iter reports a state's first output alone and never expands the copies, so duplicates
    // do not concern it): find3 for a Standard handle, left3 for a leftmost handle's shadow.
    const bool select = find3_built && fits && find3_lds_bytes(e.find3, true) <= kWorkgroupLds;
    e.find3_ok = select && !shadow;
    e.left3_ok = select && shadow && left3_lds_bytes(e.find3, true) <= kWorkgroupLds;
    // EXPAND places every further copy of a duplicate as an extra, all at the position where the pattern ends, and counts the extras of a
    // position in 4 bits (emit3_kernels.hip, kEmit3MaxExtrasAtPosition): a pattern with more further copies than that gives up every tile
    // it occurs in, so its tuples go to the segment scanners from the start.
    uint32_t max_copies = 0;
    for (const U32x4 &r : g2.erec) max_copies = std::max(max_copies, r.w >> 24);
    e.emit3_ok = fits && max_copies <= kEmit3MaxExtrasAtPosition;
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- wide GRAM: only where the 32-bit tables do not apply
template <class Sink>
daac_status gram_wide(const HostPma &h, const UploadOptions &o, EngineTables &e, Sink &sink) {
    Gram2WTables gw;
    const int64_t budget = o.gram_lds_budget - static_cast<int64_t>(kHitRingBytes);
    if (!(budget > 0 && build_gram2w_tables(h, static_cast<uint32_t>(budget), gw))) return DAAC_OK;
    Gram2WDev &d = e.gramw;
    LAYOUT_TRY(sink.put(gw.cls, d.cls));
    LAYOUT_TRY(put_as(sink, gw.m, d.m));
    LAYOUT_TRY(sink.put(gw.sdir, d.sdir));
    std::vector<uint16_t> cid(gw.cid4.size());
    for (size_t i = 0; i < cid.size(); ++i) cid[i] = static_cast<uint16_t>(kGram2OffH + gw.cid4[i]);
    LAYOUT_TRY(sink.put(cid, d.cid4));
    LAYOUT_TRY(sink.put(gw.hsum, d.hsum));
    LAYOUT_TRY(put_as(sink, gw.drec, d.drec));
    LAYOUT_TRY(put_as(sink, gw.dhit, d.dhit));
    d.m_bytes = pad16(gw.m.size() * 8); d.s_bytes = pad16(gw.sdir.size() * 4);
    d.cid_bytes = pad16(cid.size() * 2); d.h_bytes = pad16(gw.hsum.size() * 4);
    d.off_m_count = kGram2OffM;
    d.off_s_count = d.off_m_count + d.m_bytes;
    d.off_ring_count = d.off_s_count + d.s_bytes;
    d.lds_count = d.off_ring_count + kHitRingBytes;
    d.off_m_exact = kGram2OffH + d.h_bytes;
    d.off_s_exact = d.off_m_exact + d.m_bytes;
    d.off_cid = d.off_s_exact + d.s_bytes;
    d.off_ring_exact = d.off_cid + d.cid_bytes;
    d.lds_exact = d.off_ring_exact + kHitRingBytes;
    d.C = gw.C; d.unused_byte = gw.unused_byte; d.n_deep = static_cast<uint32_t>(gw.dhit.size());
    d.exact_ok = gw.exact_available && kGram2OffH + gw.hsum.size() * 4 <= 65536 && d.lds_exact <= kWorkgroupLds;
    e.gramw_ok = d.lds_count <= kWorkgroupLds;
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- PFX, with its emitter
template <class Sink>
daac_status pfx(const HostPma &h, EngineTables &e, Sink &sink) {
    PfxTables px;
    // (what the plan below leaves the three LDS tables: the per-wave areas, CNT1's companions and a margin off)
    const bool built = build_pfx_tables(h, kWorkgroupLds - 16u * (2u * 1056u + 512u) - 64u - 1024u, px);
    e.n_distinct_bytes = px.n_distinct_bytes;
    if (!built) return DAAC_OK;
    PfxDev &d = e.pfx;
    px.disp.resize((px.disp.size() + 7) & ~size_t(7), 0);
    LAYOUT_TRY(sink.put(px.bloom, d.bloom));
    LAYOUT_TRY(sink.put(px.cnt1, d.cnt1));
    LAYOUT_TRY(sink.put(px.disp, d.disp));
    LAYOUT_TRY(put_as(sink, px.slots, d.slots));
    LAYOUT_TRY(put_as(sink, px.wrec, d.wrec));
    LAYOUT_TRY(put_as(sink, px.slots_x, d.slots_x));
    LAYOUT_TRY(put_as(sink, px.wrec_x, d.wrec_x));
    LAYOUT_TRY(sink.put(px.hs1, d.hs1));
    LAYOUT_TRY(sink.put(std::vector<uint32_t>(4, 0), e.pfx_probe_word));
    if (px.emit_ok) {
        LAYOUT_TRY(put_as(sink, px.slots_e, d.slots_e));
        std::vector<uint32_t> v1f(320, 0);   // V1 by byte, then the flag bytes
        std::memcpy(v1f.data(), px.v1.data(), 1024);
        std::memcpy(v1f.data() + 256, px.has1.data(), 256);
        LAYOUT_TRY(sink.put(v1f, e.pfx_emit.v1));
        e.pfx_emit.v1_bytes = 1280;
        e.pfx_emit.K = 1;
    }
    d.G = px.G; d.has_len1 = px.has_len1; d.bloom_words = px.bloom_words; d.buckets = px.buckets; d.n_slots = px.n_slots;
    d.seed = px.seed; d.n_keys = px.n_keys;
    d.bloom_bytes = pad16(px.bloom.size() * 4);
    d.disp_bytes = pad16(px.disp.size() * 2);
    e.pfx_ok = pfx_plan(d, kWorkgroupLds);
    e.pfx_emit_ok = e.pfx_ok && px.emit_ok && h.max_pattern_len() < (1u << 22);
    return DAAC_OK;
}

// ----------------------------------------------------------------------------------- a handle's tables, in the order they are put
template <class Sink>
daac_status charwise_handle(const HostCharPma &p, const UploadOptions &o, EngineTables &e, Sink &sink) {
    OutputsDev outs;
    LAYOUT_TRY(outputs(p.outputs, outs, sink));
    return charwise(p, o, outs, e, sink);
}

template <class Sink>
daac_status bytewise_handle(const HostPma &h, const UploadOptions &o, EngineTables &e, Sink &sink) {
    OutputsDev outs;
    LAYOUT_TRY(outputs(h.outputs, outs, sink));
    LAYOUT_TRY(darray(h, outs, e, sink));
    LAYOUT_TRY(tiered(h, o, outs, e, sink));
    HostPma shadow;
    const bool have_shadow = leftmost_shadow(h, o, shadow);
    Gram2Tables g2;
    LAYOUT_TRY(gram2(have_shadow ? shadow : h, o, g2, e, sink));
    if (e.gram2_ok) LAYOUT_TRY(gram4(g2, o, e, sink));
    if (e.gram2_ok && g2.emit_available) LAYOUT_TRY(emitter(g2, have_shadow, e, sink));
    if (!e.gram_ok && !e.gram2_ok) LAYOUT_TRY(gram_wide(h, o, e, sink));
    // `.count()` for every bytewise Standard automaton the GRAM tables do not serve (any alphabet); pfx = 2 builds it always
    if (o.pfx == 2 || (o.pfx == 1 && !e.gram_ok && !e.gram2_ok && !e.gramw_ok)) LAYOUT_TRY(pfx(h, e, sink));
    return DAAC_OK;
}

#undef LAYOUT_TRY

}  // namespace layout
}  // namespace daac
