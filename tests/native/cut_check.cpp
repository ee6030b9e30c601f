// The per-lane bodies of cut_kernels.hip (daachorse_amd/csrc/cut.hpp) as plain C++ on the CPU, for a build with
// -fsanitize=address,undefined.  Every array has exactly the size the C ABI gives it, so a lane that leaves its own is an error here.
//
//   cut_check batch FILE          FILE: "B base", then per document "D len s e v s e v ..".  Prints seg_offsets, doc_segs, seg_values.
//   cut_check random ROUNDS SEED  random batches (empty documents, matches at 0 and at the document's end, adjacent matches, n = 0,
//                                 batches of only empty documents) and random token lists over their segments: the cut and the splice
//                                 (lanes = 1 and lanes = 64, with and without spans) against a sequential restatement.  Every fourth
//                                 round the tuples are hostile (ends beyond the document, overlaps, lengths beyond the end): no result
//                                 is compared, the two passes only have to stay inside their arrays.
#define DAAC_CUT_HOST
#include "../../daachorse_amd/csrc/cut.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

using namespace daac;
using u64 = unsigned long long;

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {   // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

struct Batch {
    u64 base = 0;
    std::vector<u64> len;
    std::vector<std::vector<CutTuple>> m;
};
struct Cut { std::vector<u64> so, ds; std::vector<uint32_t> sv; };

static Cut cut_by_lanes(const Batch &b) {
    const uint64_t n = b.len.size();
    std::vector<u64> off(n + 1, b.base), first(n + 1, 0);
    std::vector<CutTuple> seg;
    for (uint64_t i = 0; i < n; ++i) {
        off[i + 1] = off[i] + b.len[i];
        seg.insert(seg.end(), b.m[i].begin(), b.m[i].end());
        first[i + 1] = seg.size();
    }
    auto p_off = exact(off), p_first = exact(first);
    auto p_seg = exact(seg);
    const uint64_t items = n + seg.size();
    std::unique_ptr<u64[]> counts(new u64[items + 1]);
    CutArgs a{};
    a.seg = p_seg.get(); a.doc_first = p_first.get(); a.doc_off = p_off.get(); a.n_docs = n; a.k = seg.size(); a.counts = counts.get();
    for (uint64_t x = 0; x <= items; ++x) counts[x] = cut_count_lane(a, x);
    u64 run = 0;
    for (uint64_t x = 0; x <= items; ++x) { const u64 t = counts[x]; counts[x] = run; run += t; }
    Cut c;
    std::unique_ptr<u64[]> so(new u64[run + 1]), ds(new u64[n + 1]);
    std::unique_ptr<uint32_t[]> sv(new uint32_t[run]);
    std::memset(so.get(), 0xAB, (run + 1) * sizeof(u64));
    a.seg_offsets = so.get(); a.doc_segs = ds.get(); a.seg_values = sv.get();
    for (uint64_t x = items + 1; x-- > 0;) cut_write_lane(a, x);   // (any order)
    c.so.assign(so.get(), so.get() + run + 1);
    c.ds.assign(ds.get(), ds.get() + n + 1);
    c.sv.assign(sv.get(), sv.get() + run);
    return c;
}

static Cut cut_sequential(const Batch &b) {
    Cut c;
    u64 at = b.base;
    c.ds.push_back(0);
    for (size_t i = 0; i < b.len.size(); ++i) {
        u64 pos = 0;
        for (const CutTuple &t : b.m[i]) {
            const u64 s = t.end - t.len;
            if (s > pos) { c.so.push_back(at + pos); c.sv.push_back(kCutText); }
            c.so.push_back(at + s); c.sv.push_back(t.value);
            pos = t.end;
        }
        if (b.len[i] > pos) { c.so.push_back(at + pos); c.sv.push_back(kCutText); }
        at += b.len[i];
        c.ds.push_back(c.sv.size());
    }
    c.so.push_back(at);
    return c;
}

static int fail(const char *what, unsigned round) { std::printf("FAIL %s in round %u\n", what, round); return 1; }

static int run_batch(const char *path) {
    std::ifstream f(path);
    Batch b;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        char tag; in >> tag;
        if (tag == 'B') in >> b.base;
        if (tag != 'D') continue;
        u64 len, s, e, v; in >> len;
        b.len.push_back(len);
        b.m.emplace_back();
        while (in >> s >> e >> v) b.m.back().push_back(CutTuple{e, static_cast<uint32_t>(e - s), static_cast<uint32_t>(v)});
    }
    const Cut c = cut_by_lanes(b);
    std::printf("O"); for (u64 x : c.so) std::printf(" %llu", x);
    std::printf("\nS"); for (u64 x : c.ds) std::printf(" %llu", x);
    std::printf("\nV"); for (uint32_t x : c.sv) std::printf(" %u", x);
    std::printf("\n");
    return 0;
}

static int run_random(unsigned rounds, unsigned seed) {
    std::mt19937_64 rng(seed);
    auto below = [&](u64 n) { return n ? rng() % n : 0; };
    for (unsigned r = 0; r < rounds; ++r) {
        const bool hostile = r % 4 == 3;
        Batch b;
        b.base = below(3) ? below(1000) : 0;
        const u64 n = r % 17 == 0 ? 0 : 1 + below(12);
        const bool all_empty = r % 13 == 5;
        for (u64 i = 0; i < n; ++i) {
            const u64 len = all_empty || below(5) == 0 ? 0 : 1 + below(40);
            b.len.push_back(len);
            b.m.emplace_back();
            u64 pos = 0;
            while (pos < len && below(4)) {
                const u64 s = below(3) == 0 ? pos : pos + below(len - pos), l = 1 + below(below(3) ? 3 : len - s);
                if (s + l > len) break;
                b.m.back().push_back(CutTuple{s + l, static_cast<uint32_t>(l), static_cast<uint32_t>(below(1000))});
                pos = s + l;
            }
            if (len && below(4) == 0 && pos < len) { b.m.back().push_back(CutTuple{len, static_cast<uint32_t>(len - pos), 7u}); }   // up to the document's end
            if (hostile)
                for (u64 j = below(4); j-- > 0;)
                    b.m.back().insert(b.m.back().begin() + below(b.m.back().size() + 1), CutTuple{below(3) ? below(len + 20) : ~0ull - below(5), static_cast<uint32_t>(below(2) ? below(60) : 0xFFFFFFFFu - below(3)), 3u});
        }
        const Cut got = cut_by_lanes(b);
        if (got.ds.size() != n + 1 || got.so.size() != got.sv.size() + 1 || got.ds[n] != got.sv.size()) return fail("cut shape", r);
        if (hostile) continue;
        const Cut want = cut_sequential(b);
        if (got.so != want.so || got.ds != want.ds || got.sv != want.sv) return fail("cut", r);
        for (size_t s = 0; s + 1 < got.so.size(); ++s) if (got.so[s + 1] <= got.so[s]) return fail("an empty segment", r);
        // ---- the splice over this cut
        const uint64_t n_segs = got.sv.size();
        std::vector<u64> seg_tok(1, 0), spans, off(n + 1, b.base);
        for (u64 i = 0; i < n; ++i) off[i + 1] = off[i] + b.len[i];
        std::vector<uint32_t> ids;
        for (uint64_t s = 0; s < n_segs; ++s) {
            const u64 c = got.sv[s] == kCutText ? (below(4) ? below(6) : s % 7 == 0 ? 200 : 0) : (u64[]){0, 1, 5}[below(3)];
            for (u64 t = 0; t < c; ++t) { ids.push_back(static_cast<uint32_t>(rng())); const u64 a0 = below(30); spans.push_back(a0); spans.push_back(a0 + below(9)); }
            seg_tok.push_back(ids.size());
        }
        std::vector<uint32_t> w_ids; std::vector<u64> w_spans, w_doc(1, 0);
        for (u64 d = 0; d < n; ++d) {
            for (u64 s = got.ds[d]; s < got.ds[d + 1]; ++s) {
                const u64 delta = got.so[s] - off[d];
                if (got.sv[s] != kCutText) { w_ids.push_back(got.sv[s]); w_spans.push_back(delta); w_spans.push_back(delta + got.so[s + 1] - got.so[s]); continue; }
                for (u64 t = seg_tok[s]; t < seg_tok[s + 1]; ++t) { w_ids.push_back(ids[t]); w_spans.push_back(spans[2 * t] + delta); w_spans.push_back(spans[2 * t + 1] + delta); }
            }
            w_doc.push_back(w_ids.size());
        }
        auto p_ids = exact(ids); auto p_spans = exact(spans), p_tok = exact(seg_tok), p_so = exact(got.so), p_ds = exact(got.ds), p_off = exact(off);
        auto p_sv = exact(got.sv);
        for (int variant = 0; variant < 4; ++variant) {
            const bool want_spans = variant & 1;
            const uint32_t lanes = variant & 2 ? 64u : 1u;
            std::unique_ptr<u64[]> out_tok(new u64[n_segs + 1]);
            SpliceArgs a{};
            a.ids = p_ids.get(); a.spans = want_spans ? p_spans.get() : nullptr; a.seg_tok = p_tok.get(); a.seg_values = p_sv.get();
            a.seg_offsets = p_so.get(); a.doc_segs = p_ds.get(); a.doc_off = p_off.get(); a.n_segs = n_segs; a.n_docs = n; a.out_seg_tok = out_tok.get();
            for (uint64_t s = 0; s <= n_segs; ++s) out_tok[s] = splice_count_lane(a, s);
            u64 run = 0;
            for (uint64_t s = 0; s <= n_segs; ++s) { const u64 t = out_tok[s]; out_tok[s] = run; run += t; }
            if (run != w_ids.size()) return fail("splice total", r);
            std::unique_ptr<uint32_t[]> o_ids(new uint32_t[run]);
            std::unique_ptr<u64[]> o_spans(new u64[2 * run]);
            a.out_ids = o_ids.get(); a.out_spans = want_spans ? o_spans.get() : nullptr;
            for (uint64_t s = 0; s < n_segs; ++s)
                for (uint32_t lane = 0; lane < lanes; ++lane) splice_write_segment(a, s, lane, lanes);
            if (std::vector<uint32_t>(o_ids.get(), o_ids.get() + run) != w_ids) return fail("splice ids", r);
            if (want_spans && std::vector<u64>(o_spans.get(), o_spans.get() + 2 * run) != w_spans) return fail("splice spans", r);
            for (u64 d = 0; d <= n; ++d) if (out_tok[got.ds[d]] != w_doc[d]) return fail("doc_tok", r);   // offsets_compose
        }
    }
    std::printf("OK %u rounds\n", rounds);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "batch")) return run_batch(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "random")) return run_random(static_cast<unsigned>(std::atoi(argv[2])), static_cast<unsigned>(std::atoi(argv[3])));
    std::fprintf(stderr, "usage: cut_check batch FILE | cut_check random ROUNDS SEED\n");
    return 2;
}
