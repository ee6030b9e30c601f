// Host-side check of the upload's layout layer (daachorse_amd/csrc/upload_layout.hpp; no GPU, no HIP runtime library): builds the automaton
// of every pattern file it is given, runs the layout with the default options (or the ones named) and a sink that records instead of
// uploading, and prints one record per dictionary — tests/test_upload_layout_host.py compares the output with tests/golden/upload_layout.txt.
//   usage: upload_layout_check <name> <b|c> <match kind 0..2> <pattern file> <options> [<name> <b|c> <kind> <file> <options> ...]
//   options: `-` or option=value[,option=value...] over the defaults (the members of UploadOptions)
//   a pattern file: u32 n | u64 offsets[n + 1] | u32 values[n] | the patterns' bytes, end to end
// A record: `== name`, then for every put in order `put <index> <element bytes> <elements> <FNV-1a 64 of the bytes>`, then every *Dev struct
// and the flags, one line each, fields by name.  A pointer field is printed as the index of the put it points at (`-`: null): never an address.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../daachorse_amd/csrc/upload_layout.hpp"

using namespace daac;

namespace {

struct RecordingSink {
    struct Put { size_t elem, count; uint64_t hash; std::unique_ptr<unsigned char[]> copy; };
    std::vector<Put> puts;
    template <class T>
    daac_status put(const std::vector<T> &v, const T *&out) {
        const size_t bytes = v.size() * sizeof(T);
        std::unique_ptr<unsigned char[]> copy(new unsigned char[bytes + 16]());   // (its address stands for the device pointer)
        if (bytes) std::memcpy(copy.get(), v.data(), bytes);
        uint64_t h = 0xcbf29ce484222325ull;
        for (size_t i = 0; i < bytes; ++i) h = (h ^ copy[i]) * 0x100000001b3ull;
        out = reinterpret_cast<const T *>(copy.get());
        puts.push_back(Put{sizeof(T), v.size(), h, std::move(copy)});
        return DAAC_OK;
    }
    std::string index_of(const void *p) const {
        if (!p) return "-";
        for (size_t i = 0; i < puts.size(); ++i) if (puts[i].copy.get() == p) return std::to_string(i);
        return "?";   // (a pointer no put gave out: a bug of the layout)
    }
};

const RecordingSink *g_sink = nullptr;
#define S(st, f) std::printf(" " #f "=%" PRIu64, static_cast<uint64_t>((st).f))
#define P(st, f) std::printf(" " #f "=@%s", g_sink->index_of((st).f).c_str())

void print_emit(const char *name, const Gram2EmitDev &d) {
    std::printf("%s", name);
    P(d, cls); P(d, me); P(d, sdir); P(d, v1); P(d, v2); P(d, v3); P(d, erec); P(d, ehit); P(d, ehit4); P(d, dupo); P(d, dupv); S(d, level_start); P(d, cfirst);
    S(d, m_bytes); S(d, s_bytes); S(d, v1_bytes); S(d, v2_bytes); S(d, off_s); S(d, off_v1); S(d, off_v2); S(d, off_ring); S(d, off_wave); S(d, lds_bytes);
    S(d, K); S(d, C); S(d, s16); S(d, unused_byte); P(d, v3c); S(d, v3c_bytes); S(d, v3c_dir); S(d, v3c_val);
    std::printf("\n");
}
void print_find3(const char *name, const Find3Dev &d) {
    std::printf("%s", name);
    P(d, h1); P(d, h2); P(d, h3c); S(d, h1_bytes); S(d, h2_bytes); S(d, h3c_bytes); S(d, h3c_dir); S(d, h3c_val); S(d, C);
    std::printf("\n");
}

void print_record(const char *name, const EngineTables &e, const RecordingSink &sink) {
    g_sink = &sink;
    std::printf("== %s\n", name);
    for (size_t i = 0; i < sink.puts.size(); ++i) std::printf("put %zu %zu %zu %016" PRIx64 "\n", i, sink.puts[i].elem, sink.puts[i].count, sink.puts[i].hash);
    std::printf("flags");
    S(e, tier_ok); S(e, gram_ok); S(e, gram2_ok); S(e, gram4_ok); S(e, gramw_ok); S(e, pfx_ok); S(e, pfx_emit_ok); S(e, emit3_ok); S(e, find3_ok); S(e, left3_ok);
    S(e, emit3_has_len1); S(e, n_distinct_bytes); P(e, pfx_probe_word);
    std::printf("\n");
    { const CharDev &d = e.chr; std::printf("chr");
      P(d, states); P(d, fail_plain); P(d, table); P(d, osum); P(d, outputs); P(d, ohash); S(d, table_len); S(d, n); S(d, root_flag); S(d, leftmost);
      S(d, map_in_lds); S(d, map_lo); P(d, root_row); S(d, alphabet); S(d, row_in_lds); P(d, wstates); S(d, obits); S(d, fbits); std::printf("\n"); }
    { const DArrayDev &d = e.da; std::printf("da");
      P(d, hot); P(d, fail); P(d, fail_plain); P(d, rec); P(d, root_chain); P(d, root); P(d, osum); P(d, outputs); P(d, ohash); S(d, n); S(d, root_flag); S(d, leftmost);
      std::printf("\n"); }
    { const TierDev &d = e.tier; std::printf("tier");
      P(d, rows); P(d, bcmap); P(d, bfail); P(d, ssum); P(d, cls); P(d, grec); P(d, sopos); P(d, outputs); P(d, ohash); S(d, C); S(d, NA); S(d, NB); S(d, N);
      S(d, off_bcmap); S(d, off_bfail); S(d, off_ssum); S(d, off_cls); S(d, lds_bytes); S(d, row32); S(d, root_flag); std::printf("\n"); }
    { const TierTables &d = e.tier_host_meta; std::printf("tier_host_meta");
      S(d, available); S(d, C); S(d, N); S(d, NA); S(d, NB); S(d, dense_depth); S(d, row32); S(d, root_flag);
      std::printf(" kept=%zu\n", d.cls.size() + d.rows16.size() + d.rows32.size() + d.bcmap.size() + d.bfail.size() + d.grec.size() + d.ssum.size() + d.sopos.size() + d.old_of_new.size()); }
    { const GramDev &d = e.gram; std::printf("gram");
      P(d, cls32); P(d, cid); P(d, combo); P(d, bbits); P(d, brank); P(d, bsuper); P(d, drec); P(d, dhit); P(d, dhit4); P(d, cfirst);
      S(d, off_cid); S(d, off_combo); S(d, off_bbits); S(d, off_brank); S(d, off_bsuper); S(d, off_scratch); S(d, lds_bytes); S(d, K); S(d, C); S(d, CC); S(d, CCC);
      S(d, level_start); S(d, unused_byte); S(d, has_short); S(d, rank_in_lds); S(d, n_deep); std::printf("\n"); }
    { const Gram2Dev &d = e.gram2; std::printf("gram2");
      P(d, cls); P(d, m); P(d, sdir); P(d, rfull); P(d, cid4); P(d, hsum); P(d, drec); P(d, dhit); P(d, dhit4); P(d, cfirst);
      S(d, m_bytes); S(d, s_bytes); S(d, cid_bytes); S(d, h_bytes); S(d, off_m_count); S(d, off_s_count); S(d, off_ring_count); S(d, lds_count);
      S(d, rfull_bytes); S(d, off_ring_rfull); S(d, lds_rfull); S(d, rfull_ok); S(d, off_m_exact); S(d, off_s_exact); S(d, off_cid); S(d, off_ring_exact); S(d, lds_exact);
      S(d, K); S(d, C); S(d, s16); S(d, unused_byte); S(d, n_deep); S(d, exact_ok); S(d, xlane_dpp); std::printf("\n"); }
    { const Gram4Dev &d = e.gram4; std::printf("gram4");
      P(d, cls); P(d, m); P(d, rfull); P(d, sdir); P(d, dhit_c); P(d, dhit_t); P(d, drec_c); P(d, drec_t); P(d, bloom); S(d, bloom_words); P(d, mph_disp); P(d, dhit_h);
      S(d, mph.bk8); S(d, mph.nh); S(d, mph.shift); S(d, mph.a); S(d, mph.b); S(d, mph_bytes); S(d, m_bytes); S(d, rfull_bytes); S(d, s_bytes);
      S(d, K); S(d, C); S(d, s16); S(d, arith); S(d, lo); S(d, unused_byte); S(d, n_deep); std::printf("\n"); }
    { const Gram2WDev &d = e.gramw; std::printf("gramw");
      P(d, cls); P(d, m); P(d, sdir); P(d, cid4); P(d, hsum); P(d, drec); P(d, dhit); S(d, m_bytes); S(d, s_bytes); S(d, cid_bytes); S(d, h_bytes);
      S(d, off_m_count); S(d, off_s_count); S(d, off_ring_count); S(d, lds_count); S(d, off_m_exact); S(d, off_s_exact); S(d, off_cid); S(d, off_ring_exact); S(d, lds_exact);
      S(d, C); S(d, unused_byte); S(d, n_deep); S(d, exact_ok); std::printf("\n"); }
    print_emit("emit", e.emit);
    { const Gram3Lds &d = e.emit3_lds; std::printf("emit3_lds");
      S(d, off_s); S(d, off_wave); S(d, wave_stride); S(d, lds_bytes); S(d, threads); S(d, rfull); std::printf("\n"); }
    print_find3("find3", e.find3);
    print_find3("find3v", e.find3v);
    { const PfxDev &d = e.pfx; std::printf("pfx");
      P(d, bloom); P(d, cnt1); P(d, disp); P(d, slots); P(d, wrec); P(d, slots_x); P(d, wrec_x); P(d, hs1); P(d, slots_e);
      S(d, G); S(d, has_len1); S(d, bloom_words); S(d, buckets); S(d, n_slots); S(d, seed); S(d, bloom_bytes); S(d, disp_bytes);
      S(d, off_disp); S(d, off_cnt1); S(d, off_wave); S(d, wave_stride); S(d, lds_bytes); S(d, threads); S(d, n_keys); std::printf("\n"); }
    print_emit("pfx_emit", e.pfx_emit);
}

// the defaults of DAAC_OPTIONS (api_internal.hpp), then `spec`
bool parse_options(const char *spec, UploadOptions &o) {
    o = UploadOptions{};
    o.lds_budget = 96 * 1024; o.dense_depth = -1; o.rows_share_pct = 45;
    o.gram_lds_budget = 158 * 1024; o.gram_rank_in_lds = -1;
    o.gram4_mph = 8; o.gram2_rfull = 1; o.gram2_dpp = 1;
    o.left3 = 1; o.pfx = 1;
    o.char_map_lds = 1; o.char_row_lds = 1;
    const struct { const char *name; int64_t UploadOptions::*field; } known[] = {
#define O(f) {#f, &UploadOptions::f}
        O(lds_budget), O(dense_depth), O(rows_share_pct), O(gram_lds_budget), O(gram_rank_in_lds), O(gram4_mph), O(gram2_rfull), O(gram2_dpp), O(left3), O(pfx),
        O(char_map_lds), O(char_row_lds)};
#undef O
    std::string s(spec);
    if (s == "-") return true;
    for (size_t at = 0; at < s.size();) {
        const size_t end = std::min(s.find(',', at), s.size()), eq = s.find('=', at);
        if (eq == std::string::npos || eq >= end) return false;
        bool found = false;
        for (const auto &k : known) if (s.compare(at, eq - at, k.name) == 0) { o.*k.field = std::atoll(s.c_str() + eq + 1); found = true; }
        if (!found) return false;
        at = end + 1;
    }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 6 || (argc - 1) % 5 != 0) { std::fprintf(stderr, "usage: upload_layout_check <name> <b|c> <match kind> <pattern file> <options> ...\n"); return 2; }
    for (int a = 1; a < argc; a += 5) {
        std::ifstream f(argv[a + 3], std::ios::binary);
        const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        uint32_t n = 0;
        if (!f.good() && !f.eof()) { std::fprintf(stderr, "%s: unreadable\n", argv[a + 3]); return 2; }
        if (raw.size() < 4) { std::fprintf(stderr, "%s: too short\n", argv[a + 3]); return 2; }
        std::memcpy(&n, raw.data(), 4);
        const size_t head = 4 + (static_cast<size_t>(n) + 1) * 8 + static_cast<size_t>(n) * 4;
        if (raw.size() < head) { std::fprintf(stderr, "%s: too short\n", argv[a + 3]); return 2; }
        std::vector<uint64_t> offs(n + 1);
        std::vector<uint32_t> vals(n);
        std::memcpy(offs.data(), raw.data() + 4, offs.size() * 8);
        if (n) std::memcpy(vals.data(), raw.data() + 4 + offs.size() * 8, vals.size() * 4);
        if (offs[n] != raw.size() - head) { std::fprintf(stderr, "%s: offsets and bytes disagree\n", argv[a + 3]); return 2; }
        const uint8_t *blob = reinterpret_cast<const uint8_t *>(raw.data()) + head;
        const uint8_t kind = static_cast<uint8_t>(std::atoi(argv[a + 2]));
        UploadOptions opt;
        if (!parse_options(argv[a + 4], opt)) { std::fprintf(stderr, "%s: bad options %s\n", argv[a], argv[a + 4]); return 2; }
        EngineTables e;
        RecordingSink sink;
        daac_status st;
        if (argv[a + 1][0] == 'c') {
            HostCharPma p;
            if ((st = build_charwise(blob, offs.data(), vals.data(), n, kind, 16, p)) != DAAC_OK) { std::fprintf(stderr, "%s: build_charwise %d: %s\n", argv[a], st, last_error_cstr()); return 1; }
            st = layout::charwise_handle(p, opt, e, sink);
        } else {
            HostPma p;
            if ((st = build_bytewise(blob, offs.data(), vals.data(), n, kind, 16, p)) != DAAC_OK) { std::fprintf(stderr, "%s: build_bytewise %d: %s\n", argv[a], st, last_error_cstr()); return 1; }
            st = layout::bytewise_handle(p, opt, e, sink);
        }
        if (st != DAAC_OK) { std::fprintf(stderr, "%s: layout %d\n", argv[a], st); return 1; }
        print_record(argv[a], e, sink);
    }
    return 0;
}
