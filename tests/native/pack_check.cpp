// The per-lane bodies of pack_kernels.hip (daachorse_amd/csrc/pack.hpp) as plain C++ on the CPU, for a build with
// -fsanitize=address,undefined.  Every array has exactly the size the C ABI gives it, so a lane that leaves its own is an error here.
//
//   pack_check batch FILE          FILE: "P n_pieces {kind id type_id}..", "C truncate budget strategy trunc_left padding pad_length
//                                  pad_multiple pad_left pad_id pad_type_id width pair", then per document "A n {id start end}.." and,
//                                  for pairs, "B n {id start end}..".  Prints "E doc why" for the first document in error, or "L row
//                                  slots" and the planes I, T, M (dense only), S, O and, for the CSR form, R.
//   pack_check random ROUNDS SEED  random templates, strategies, sides, paddings and widths over random batches (empty documents, n = 0,
//                                  pairs that cannot be truncated) against a sequential restatement; every fourth round the offsets are
//                                  hostile (they decrease or leave the token list): the header pass has to name the first such document
//                                  and to stay inside its arrays.
#define DAAC_PACK_HOST
#include "../../daachorse_amd/csrc/pack.hpp"

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

struct Seq {
    std::vector<uint32_t> ids;
    std::vector<u64> spans, off{0};
};
struct Config {
    std::vector<PackPiece> pieces;
    uint32_t truncate = 0, strategy = 0, trunc_left = 0, padding = 1, pad_left = 0, pad_id = 0, pad_type_id = 0, width = 8;
    u64 budget = 0, pad_length = 0, pad_multiple = 1;
    bool pair = false;
};
struct Result {
    bool error = false;
    u64 doc = 0, why = 0, L = 0, slots = 0;
    std::vector<u64> ids, types, attention, special, offsets, row_offsets;
};

static std::vector<u64> plane_values(const void *p, uint32_t width, u64 n) {
    std::vector<u64> v(n);
    for (u64 i = 0; i < n; ++i) v[i] = width == 8 ? static_cast<const uint64_t *>(p)[i] : static_cast<const uint32_t *>(p)[i];
    return v;
}

// what api_pack.hip does around the two passes
static Result pack_by_lanes(const Config &c, const Seq &sa, const Seq &sb) {
    const u64 n = sa.off.size() - 1;
    auto a_ids = exact(sa.ids), b_ids = exact(sb.ids);
    auto a_sp = exact(sa.spans), b_sp = exact(sb.spans), a_off = exact(sa.off), b_off = exact(sb.off);
    PackArgs a{};
    a.a_ids = a_ids.get(); a.a_spans = a_sp.get(); a.a_off = a_off.get(); a.a_tokens = sa.ids.size();
    if (c.pair) { a.b_ids = b_ids.get(); a.b_spans = b_sp.get(); a.b_off = b_off.get(); a.b_tokens = sb.ids.size(); }
    a.n_docs = n;
    a.n_pieces = static_cast<uint32_t>(c.pieces.size());
    for (size_t i = 0; i < c.pieces.size(); ++i) {
        a.pieces[i] = c.pieces[i];
        a.n_added += c.pieces[i].kind == kPackSpecial;
    }
    a.truncate = c.truncate; a.strategy = c.strategy; a.trunc_left = c.truncate ? c.trunc_left : 0; a.budget = c.budget;
    const bool csr = c.padding == 0;
    a.pad_left = csr ? 0 : c.pad_left; a.pad_id = c.pad_id; a.pad_type_id = c.pad_type_id; a.width = c.width; a.csr = csr;
    std::unique_ptr<u64[]> hdr(new u64[kPackHdrWords * n]), row_len(new u64[n + 1]);
    a.hdr = hdr.get();
    a.row_len = csr ? row_len.get() : nullptr;
    Result r;
    u64 longest = 0, code = ~0ull;
    for (u64 d = n; d-- > 0;) {   // (any order)
        const PackRow row = pack_header_lane(a, d);
        longest = row.row_len > longest ? row.row_len : longest;
        r.slots += row.row_len;
        if (row.error && 2 * d + row.why < code) code = 2 * d + row.why;
    }
    if (code != ~0ull) { r.error = true; r.doc = code / 2; r.why = code % 2; return r; }
    r.L = longest;
    if (csr) {
        u64 run = 0;
        row_len[n] = 0;
        for (u64 d = 0; d <= n; ++d) { const u64 t = row_len[d]; row_len[d] = run; run += t; }
        r.row_offsets.assign(row_len.get(), row_len.get() + n + 1);
    } else {
        if (c.padding == 2 && c.pad_length > r.L) r.L = c.pad_length;
        if (r.L % c.pad_multiple) r.L += c.pad_multiple - r.L % c.pad_multiple;
        r.slots = n * r.L;
    }
    a.L = r.L; a.slots = r.slots; a.row_offsets = row_len.get();
    const size_t bytes = r.slots * c.width;
    std::unique_ptr<unsigned char[]> ii(new unsigned char[bytes]), ti(new unsigned char[bytes]), am(new unsigned char[bytes]), sm(new unsigned char[bytes]);
    std::unique_ptr<u64[]> of(new u64[2 * r.slots]);
    std::memset(ii.get(), 0xAB, bytes);
    a.input_ids = ii.get(); a.type_ids = ti.get(); a.attention = csr ? nullptr : am.get(); a.special = sm.get(); a.offsets = of.get();
    for (u64 x = r.slots; x-- > 0;) pack_slot_lane(a, x);
    r.ids = plane_values(ii.get(), c.width, r.slots);
    r.types = plane_values(ti.get(), c.width, r.slots);
    if (!csr) r.attention = plane_values(am.get(), c.width, r.slots);
    r.special = plane_values(sm.get(), c.width, r.slots);
    r.offsets.assign(of.get(), of.get() + 2 * r.slots);
    return r;
}

// the definition, document by document
static Result pack_sequential(const Config &c, const Seq &sa, const Seq &sb) {
    const u64 n = sa.off.size() - 1;
    Result r;
    u64 n_added = 0;
    for (const PackPiece &p : c.pieces) n_added += p.kind == kPackSpecial;
    struct Slot { u64 id, type, attention, special, s, e; };
    std::vector<std::vector<Slot>> rows(n);
    for (u64 d = 0; d < n; ++d) {
        const u64 a0 = sa.off[d], n1 = sa.off[d + 1] - a0, b0 = c.pair ? sb.off[d] : 0, n2 = c.pair ? sb.off[d + 1] - b0 : 0;
        u64 k1 = n1, k2 = n2;
        if (c.truncate) {
            if (c.budget == 0) k1 = k2 = 0;
            else if (!c.pair) k1 = n1 < c.budget ? n1 : c.budget;
            else if (n1 + n2 > c.budget) {
                const u64 need = n1 + n2 - c.budget;
                if (c.strategy == kPackLongestFirst) {
                    u64 lo = n1 < n2 ? n1 : n2, hi;
                    hi = lo > c.budget ? lo : (lo > c.budget - lo ? lo : c.budget - lo);
                    if (lo + hi > c.budget) { lo = c.budget / 2; hi = lo + c.budget % 2; }
                    k1 = n1 > n2 ? hi : lo;
                    k2 = n1 > n2 ? lo : hi;
                } else if (c.strategy == kPackOnlyFirst) {
                    if (n1 <= need) { r.error = true; r.doc = d; r.why = kPackTooShort; return r; }
                    k1 = n1 - need;
                } else {
                    if (n2 <= need) { r.error = true; r.doc = d; r.why = kPackTooShort; return r; }
                    k2 = n2 - need;
                }
            }
        }
        const u64 a_first = a0 + (c.truncate && c.trunc_left ? n1 - k1 : 0), b_first = b0 + (c.truncate && c.trunc_left ? n2 - k2 : 0);
        for (const PackPiece &p : c.pieces) {
            if (p.kind == kPackSpecial) rows[d].push_back({p.id, p.type_id, 1, 1, 0, 0});
            else if (p.kind == kPackA) for (u64 t = a_first; t < a_first + k1; ++t) rows[d].push_back({sa.ids[t], p.type_id, 1, 0, sa.spans[2 * t], sa.spans[2 * t + 1]});
            else for (u64 t = b_first; t < b_first + k2; ++t) rows[d].push_back({sb.ids[t], p.type_id, 1, 0, sb.spans[2 * t], sb.spans[2 * t + 1]});
        }
        if (rows[d].size() != k1 + k2 + n_added) std::abort();
        r.L = rows[d].size() > r.L ? rows[d].size() : r.L;
    }
    if (c.padding != 0) {
        if (c.padding == 2 && c.pad_length > r.L) r.L = c.pad_length;
        r.L = (r.L + c.pad_multiple - 1) / c.pad_multiple * c.pad_multiple;
        const Slot pad{c.pad_id, c.pad_type_id, 0, 1, 0, 0};
        for (auto &row : rows) row.insert(c.pad_left ? row.begin() : row.end(), r.L - row.size(), pad);
    } else r.row_offsets.push_back(0);
    for (auto &row : rows) {
        for (const Slot &s : row) {
            r.ids.push_back(s.id); r.types.push_back(s.type); r.special.push_back(s.special);
            if (c.padding != 0) r.attention.push_back(s.attention);
            r.offsets.push_back(s.s); r.offsets.push_back(s.e);
        }
        if (c.padding == 0) r.row_offsets.push_back(r.ids.size());
    }
    r.slots = r.ids.size();
    return r;
}

static void print(const char *tag, const std::vector<u64> &v) {
    std::printf("%s", tag);
    for (u64 x : v) std::printf(" %llu", x);
    std::printf("\n");
}

static int run_batch(const char *path) {
    std::ifstream f(path);
    Config c;
    Seq sa, sb;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tag;
        in >> tag;
        if (tag == "P") {
            size_t n; in >> n;
            c.pieces.resize(n);
            for (auto &p : c.pieces) in >> p.kind >> p.id >> p.type_id;
        } else if (tag == "C") {
            int pair;
            in >> c.truncate >> c.budget >> c.strategy >> c.trunc_left >> c.padding >> c.pad_length >> c.pad_multiple >> c.pad_left >> c.pad_id >> c.pad_type_id >> c.width >> pair;
            c.pair = pair != 0;
        } else if (tag == "A" || tag == "B") {
            Seq &s = tag == "A" ? sa : sb;
            size_t n; in >> n;
            for (size_t i = 0; i < n; ++i) { uint32_t id; u64 st, en; in >> id >> st >> en; s.ids.push_back(id); s.spans.push_back(st); s.spans.push_back(en); }
            s.off.push_back(s.ids.size());
        }
    }
    if (c.pieces.empty() || c.pieces.size() > kPackMaxPieces || (c.pair && sb.off.size() != sa.off.size())) { std::fprintf(stderr, "bad file\n"); return 2; }
    const Result r = pack_by_lanes(c, sa, sb);
    if (r.error) { std::printf("E %llu %llu\n", r.doc, r.why); return 0; }
    std::printf("L %llu %llu\n", r.L, r.slots);
    print("I", r.ids); print("T", r.types);
    if (c.padding != 0) print("M", r.attention);
    print("S", r.special); print("O", r.offsets);
    if (c.padding == 0) print("R", r.row_offsets);
    return 0;
}

static bool same(const Result &x, const Result &y) {
    if (x.error != y.error) return false;
    if (x.error) return x.doc == y.doc && x.why == y.why;
    return x.L == y.L && x.slots == y.slots && x.ids == y.ids && x.types == y.types && x.attention == y.attention && x.special == y.special &&
           x.offsets == y.offsets && x.row_offsets == y.row_offsets;
}

static int run_random(long rounds, unsigned long seed) {
    std::mt19937_64 rng(seed);
    auto below = [&](u64 n) { return static_cast<u64>(rng() % n); };
    for (long round = 0; round < rounds; ++round) {
        Config c;
        c.pair = below(2);
        const uint32_t n_special = static_cast<uint32_t>(below(c.pair ? 15 : 16));
        std::vector<PackPiece> pieces;
        for (uint32_t i = 0; i < n_special; ++i) pieces.push_back({kPackSpecial, static_cast<uint32_t>(1000 + below(10)), static_cast<uint32_t>(below(3))});
        pieces.insert(pieces.begin() + below(pieces.size() + 1), PackPiece{kPackA, 0, static_cast<uint32_t>(below(3))});
        if (c.pair) pieces.insert(pieces.begin() + below(pieces.size() + 1), PackPiece{kPackB, 0, static_cast<uint32_t>(below(3))});
        c.pieces = pieces;
        c.truncate = below(4) != 0;
        c.budget = below(4) == 0 ? 0 : below(12);
        c.strategy = c.pair ? static_cast<uint32_t>(below(3)) : static_cast<uint32_t>(below(2));
        c.trunc_left = below(2);
        c.padding = static_cast<uint32_t>(below(3));
        c.pad_length = below(40);
        c.pad_multiple = below(3) ? 1 : 1 + below(9);
        c.pad_left = below(2);
        c.pad_id = 7; c.pad_type_id = static_cast<uint32_t>(below(2));
        c.width = below(2) ? 8 : 4;
        const u64 n = below(5) == 0 ? 0 : 1 + below(below(8) == 0 ? 300 : 12);
        Seq sa, sb;
        for (Seq *s : {&sa, &sb})
            for (u64 d = 0; d < n; ++d) {
                const u64 len = below(3) == 0 ? 0 : below(14);
                for (u64 t = 0; t < len; ++t) { s->ids.push_back(static_cast<uint32_t>(rng())); const u64 st = below(1000); s->spans.push_back(st); s->spans.push_back(st + below(9)); }
                s->off.push_back(s->ids.size());
            }
        if (round % 4 == 3 && n) {   // hostile offsets: the first broken document is the answer
            Seq &s = c.pair && below(2) ? sb : sa;
            const u64 d = 1 + below(n);
            s.off[d] = below(2) ? s.ids.size() + 1 + below(5) : (s.off[d - 1] ? s.off[d - 1] - 1 : s.ids.size() + 1);
            const Result r = pack_by_lanes(c, sa, sb);
            // document d - 1 ends at the broken entry; an earlier document may be one that cannot be truncated
            if (!r.error || r.doc > d - 1 || (r.doc == d - 1 && r.why != kPackOffsetsBroken)) { std::printf("round %ld: hostile offsets at %llu not named (doc %llu)\n", round, d, r.doc); return 1; }
            continue;
        }
        if (!same(pack_by_lanes(c, sa, sb), pack_sequential(c, sa, sb))) { std::printf("round %ld differs\n", round); return 1; }
    }
    std::printf("OK %ld rounds\n", rounds);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "batch")) return run_batch(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "random")) return run_random(std::atol(argv[2]), std::strtoul(argv[3], nullptr, 10));
    std::fprintf(stderr, "usage: pack_check batch FILE | pack_check random ROUNDS SEED\n");
    return 2;
}
