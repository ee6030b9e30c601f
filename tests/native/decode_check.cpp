// The per-lane bodies of decode_kernels.hip (daachorse_amd/csrc/decode.hpp) as plain C++ on the CPU, for a build with
// -fsanitize=address,undefined.  Every array has exactly the size the C ABI gives it, so a lane that leaves its own is an error here.
//
//   decode_check batch FILE          FILE: "T n_ids", then per id "flags rest first" (hex, "-" for no byte), then any number of batches:
//                                    "C width dense skip_special unknown_skip row_length n_docs" and per document "D n id..".  A CSR
//                                    batch takes its offsets from the documents' lengths; a dense one has n = row_length in every
//                                    document.  Prints per batch "E doc" (offsets in error), "U token" (the lowest token without an
//                                    entry) or "O text-hex" ("-": no byte), "F out_offsets.." and "S token_starts..".
//   decode_check random ROUNDS SEED  random tables (empty images in runs, an image longer than a tile), CSR and dense batches of both
//                                    widths against a sequential restatement; hostile rounds have tiles with more tokens than the
//                                    stage holds, unknown ids (beyond the table, absent, negative, 2^32), and offsets that decrease or
//                                    leave the token list: the header pass has to name the first such document and every pass has to
//                                    stay inside its arrays.
#define DAAC_DECODE_HOST
#include "../../daachorse_amd/csrc/decode.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

using namespace daac;
using u64 = unsigned long long;
using Bytes = std::vector<uint8_t>;

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T> &v) {   // a heap block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

struct Table {
    std::vector<Bytes> rest, first;
    std::vector<uint8_t> flags;
};
struct Batch {
    uint32_t width = 4;
    bool dense = false, skip_special = true, unknown_skip = false;
    u64 row_len = 0, n_docs = 0;
    std::vector<long long> ids;   // as the caller's elements: a 4-byte one is its low 32 bits
    std::vector<u64> off;         // CSR: n_docs + 1, as given (hostile rounds break them)
};
struct Result {
    int status = 0;   // 0: text, 1: a document's offsets, 2: a token without an entry
    u64 where = 0;
    Bytes out;
    std::vector<u64> out_offsets, starts;
    bool operator==(const Result &o) const { return status == o.status && where == o.where && out == o.out && out_offsets == o.out_offsets && starts == o.starts; }
};

static u64 g_unstaged_tiles = 0;   // tiles with more tokens than the stage holds that the copy has met

// what api_decode.hip does around the passes
static Result decode_by_lanes(const Table &t, const Batch &b) {
    Result r;
    std::vector<DecodePiece> pieces(t.rest.size());
    Bytes pool;
    for (size_t i = 0; i < t.rest.size(); ++i) {
        pieces[i] = DecodePiece{static_cast<uint32_t>(pool.size()), static_cast<uint32_t>(t.rest[i].size()), 0, static_cast<uint32_t>(t.first[i].size())};
        pool.insert(pool.end(), t.rest[i].begin(), t.rest[i].end());
        pieces[i].first_off = static_cast<uint32_t>(pool.size());
        pool.insert(pool.end(), t.first[i].begin(), t.first[i].end());
    }
    const u64 T = b.ids.size();
    std::vector<uint32_t> ids4(T);
    std::vector<uint64_t> ids8(T);
    for (u64 i = 0; i < T; ++i) { ids4[i] = static_cast<uint32_t>(b.ids[i]); ids8[i] = static_cast<uint64_t>(b.ids[i]); }
    auto p_ids4 = exact(ids4);
    auto p_ids8 = exact(ids8);
    auto p_off = exact(b.off);
    auto p_pieces = exact(pieces);
    auto p_flags = exact(t.flags);
    auto p_pool = exact(pool);
    std::unique_ptr<u64[]> start(new u64[T + 1]), out_offsets(new u64[b.n_docs + 1]);
    std::unique_ptr<uint8_t[]> mark(new uint8_t[T]);
    u64 fold[kDecodeFoldWords] = {0, 0, 0};
    DecodeArgs a{};
    a.ids = b.width == 8 ? static_cast<const void *>(p_ids8.get()) : static_cast<const void *>(p_ids4.get());
    a.width = b.width;
    a.off = b.dense ? nullptr : p_off.get();
    a.row_len = b.dense ? b.row_len : 0;
    a.n_tokens = T;
    a.n_docs = b.n_docs;
    a.skip_special = b.skip_special;
    a.unknown_skip = b.unknown_skip;
    a.pieces = p_pieces.get();
    a.flags = p_flags.get();
    a.pool = p_pool.get();
    a.pool_bytes = pool.size();
    a.n_ids = pieces.size();
    a.start = start.get();
    a.mark = mark.get();
    a.fold = fold;
    a.out_offsets = out_offsets.get();
    // sizing: one lane per token, and the closing entry
    uint64_t lo, hi;
    decode_span(a, lo, hi);
    for (u64 i = 0; i < T; ++i) {
        const DecodeSized s = decode_size_lane(a, i, lo, hi);
        fold[2] += s.kept;
        if (s.unknown && ~i > fold[1]) fold[1] = ~i;
    }
    start[T] = 0;
    for (u64 d = 0; d < b.n_docs; ++d)
        if (!decode_header_lane(a, d) && ~d > fold[0]) fold[0] = ~d;
    u64 sum = 0;
    for (u64 i = 0; i <= T; ++i) { const u64 v = start[i]; start[i] = sum; sum += v; }
    if (fold[0]) { r.status = 1; r.where = ~fold[0]; return r; }
    if (fold[1] && !b.unknown_skip) { r.status = 2; r.where = ~fold[1]; return r; }
    for (u64 d = 0; d <= b.n_docs; ++d) decode_doc_offset_lane(a, d);
    r.out_offsets.assign(out_offsets.get(), out_offsets.get() + b.n_docs + 1);
    r.starts.assign(start.get(), start.get() + T + 1);
    std::unique_ptr<uint8_t[]> out(new uint8_t[sum]);
    for (u64 i = 0; i < sum; ++i) out[i] = 0xEE;
    a.out = out.get();
    a.out_len = sum;
    a.tiles = (sum + kDecodeTile - 1) / kDecodeTile;
    std::unique_ptr<long long[]> tile_lo(new long long[a.tiles + 1]);
    a.tile_lo = tile_lo.get();
    if (a.tiles) {
        for (u64 tl = 0; tl <= a.tiles; ++tl) decode_tile_lane(a, tl);
        std::unique_ptr<uint16_t[]> s_rel(new uint16_t[kDecodeStage]);
        for (u64 tl = 0; tl < a.tiles; ++tl) {
            const u64 tile_begin = tl * kDecodeTile;
            long long k_lo;
            const u64 m = decode_tile_tokens(a, tl, k_lo);
            if (m <= kDecodeStage) {
                for (u64 j = 0; j < m; ++j) s_rel[j] = static_cast<uint16_t>(a.start[k_lo + 1 + static_cast<long long>(j)] - tile_begin);
                for (uint32_t lane = 0; lane < kDecodeLanes; ++lane) decode_copy_lane<true>(a, s_rel.get(), tile_begin, k_lo, m, lane);
            } else {
                ++g_unstaged_tiles;
                for (uint32_t lane = 0; lane < kDecodeLanes; ++lane) decode_copy_lane<false>(a, nullptr, tile_begin, k_lo, m, lane);
            }
        }
    }
    r.out.assign(out.get(), out.get() + sum);
    return r;
}

// the definition, token by token
static Result decode_in_order(const Table &t, const Batch &b) {
    Result r;
    const u64 T = b.ids.size();
    std::vector<u64> t0(b.n_docs), t1(b.n_docs);
    for (u64 d = 0; d < b.n_docs; ++d) {
        if (b.dense) { t0[d] = d * b.row_len; t1[d] = t0[d] + b.row_len; continue; }
        t0[d] = b.off[d];
        t1[d] = b.off[d + 1];
        if (t1[d] < t0[d] || t1[d] > T) { r.status = 1; r.where = d; return r; }
    }
    auto known = [&](long long v, uint32_t &id) {
        if (b.width == 4) id = static_cast<uint32_t>(v);
        else { if (v < 0 || v > 0xFFFFFFFFll) return false; id = static_cast<uint32_t>(v); }
        return id < t.rest.size() && !(t.flags[id] & kDecodeAbsent);
    };
    r.starts.assign(T + 1, 0);
    std::vector<u64> len(T, 0);
    std::vector<const Bytes *> img(T, nullptr);
    bool bad = false;
    u64 first_bad = 0;
    for (u64 d = 0; d < b.n_docs; ++d) {
        bool seen = false;
        for (u64 i = t0[d]; i < t1[d]; ++i) {
            uint32_t id;
            if (!known(b.ids[i], id)) { if (!bad || i < first_bad) { bad = true; first_bad = i; } continue; }
            if ((t.flags[id] & kDecodeSpecial) && b.skip_special) continue;
            img[i] = seen ? &t.rest[id] : &t.first[id];
            len[i] = img[i]->size();
            seen = true;
        }
    }
    if (bad && !b.unknown_skip) { r.status = 2; r.where = first_bad; r.starts.clear(); return r; }
    u64 at = 0;
    for (u64 i = 0; i < T; ++i) {
        r.starts[i] = at;
        if (img[i]) r.out.insert(r.out.end(), img[i]->begin(), img[i]->end());
        at += len[i];
    }
    r.starts[T] = at;
    r.out_offsets.resize(b.n_docs + 1);
    for (u64 d = 0; d < b.n_docs; ++d) r.out_offsets[d] = r.starts[t0[d]];
    r.out_offsets[b.n_docs] = b.dense || !b.n_docs ? at : r.starts[b.off[b.n_docs]];
    return r;
}

static Bytes unhex(const std::string &s) {
    Bytes v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back(static_cast<uint8_t>(std::stoul(s.substr(i, 2), nullptr, 16)));
    return v;
}

static void print_result(const Result &r) {
    if (r.status == 1) { std::printf("E %llu\n", r.where); return; }
    if (r.status == 2) { std::printf("U %llu\n", r.where); return; }
    std::printf("O ");
    if (r.out.empty()) std::printf("-");
    for (uint8_t c : r.out) std::printf("%02x", c);
    std::printf("\nF");
    for (u64 v : r.out_offsets) std::printf(" %llu", v);
    std::printf("\nS");
    for (u64 v : r.starts) std::printf(" %llu", v);
    std::printf("\n");
}

static int run_batch(const char *path) {
    std::ifstream f(path);
    std::string tag;
    size_t n_ids = 0;
    if (!(f >> tag >> n_ids) || tag != "T") { std::fprintf(stderr, "no table\n"); return 2; }
    Table t;
    for (size_t i = 0; i < n_ids; ++i) {
        unsigned flags;
        std::string rest, first;
        f >> flags >> rest >> first;
        t.flags.push_back(static_cast<uint8_t>(flags));
        t.rest.push_back(unhex(rest));
        t.first.push_back(unhex(first));
    }
    while (f >> tag) {
        if (tag != "C") { std::fprintf(stderr, "expected C\n"); return 2; }
        Batch b;
        int dense, skip, uskip;
        f >> b.width >> dense >> skip >> uskip >> b.row_len >> b.n_docs;
        b.dense = dense; b.skip_special = skip; b.unknown_skip = uskip;
        b.off.push_back(0);
        for (u64 d = 0; d < b.n_docs; ++d) {
            u64 n;
            f >> tag >> n;
            for (u64 i = 0; i < n; ++i) { long long v; f >> v; b.ids.push_back(v); }
            b.off.push_back(b.ids.size());
        }
        const Result got = decode_by_lanes(t, b), want = decode_in_order(t, b);
        if (!(got == want)) { std::fprintf(stderr, "the lanes and the restatement differ\n"); return 1; }
        print_result(got);
    }
    return 0;
}

static int run_random(long rounds, unsigned long seed) {
    std::mt19937_64 rng(seed);
    auto rnd = [&](u64 n) { return static_cast<u64>(rng() % n); };
    u64 bytes = 0, errors = 0;
    for (long round = 0; round < rounds; ++round) {
        const bool hostile = round % 4 == 3, heavy = round % 50 == 7;
        Table t;
        const size_t n_ids = 1 + rnd(40);
        for (size_t i = 0; i < n_ids; ++i) {
            const u64 kind = rnd(10);
            const size_t len = kind < 3 ? 0 : kind < 5 ? 1 : rnd(41);
            Bytes img(len), fst;
            for (auto &c : img) c = static_cast<uint8_t>(rng());
            if (rnd(2)) { fst.resize(rnd(8)); for (auto &c : fst) c = static_cast<uint8_t>(rng()); } else { fst = img; }
            t.rest.push_back(img);
            t.first.push_back(fst);
            const uint32_t special = rnd(5) == 0 ? kDecodeSpecial : 0u, absent = hostile && rnd(12) == 0 ? kDecodeAbsent : 0u;
            t.flags.push_back(static_cast<uint8_t>(special | absent));
        }
        if (heavy) {   // an image longer than a tile, with a pattern that depends on the position
            Bytes big(5000);
            for (size_t i = 0; i < big.size(); ++i) big[i] = static_cast<uint8_t>(i * 7 + (i >> 8));
            t.rest[0] = big;
            t.flags[0] = 0;
            if (n_ids > 2) {   // an empty image and one of a byte, for the runs below
                t.rest[1].clear();
                t.rest[2].assign(1, 0x5A);
                t.flags[1] = t.flags[2] = 0;
            }
        }
        Batch b;
        b.width = rnd(2) ? 8 : 4;
        b.dense = rnd(2);
        b.skip_special = rnd(2);
        b.unknown_skip = rnd(2);
        b.n_docs = rnd(8) == 0 ? 0 : 1 + rnd(heavy ? 4 : 12);
        if (!b.dense) b.width = 4;
        b.row_len = b.dense ? 1 + rnd(heavy ? 8000 : 20) : 0;
        b.off.push_back(0);
        for (u64 d = 0; d < b.n_docs; ++d) {
            u64 n = b.dense ? b.row_len : (rnd(4) == 0 ? 0 : rnd(heavy ? 8000 : 24));
            // hostile and heavy: runs of tokens with 1-byte or empty images, more than the stage holds in a tile
            const bool run = heavy && rnd(2);
            for (u64 i = 0; i < n; ++i) {
                long long v = static_cast<long long>(rnd(n_ids));
                if (run) v = n_ids > 2 ? (rnd(3) == 0 ? 2 : 1) : 0;   // two empty images to one of a byte: more starts in a tile than the stage holds
                if (hostile && rnd(40) == 0) {
                    const u64 how = rnd(4);
                    v = how == 0 ? static_cast<long long>(n_ids + rnd(5)) : how == 1 ? -100 : how == 2 ? (1ll << 32) : (1ll << 32) + static_cast<long long>(rnd(n_ids));
                    if (b.width == 4 && how != 0) v = 0xFFFFFFFFll;
                }
                b.ids.push_back(v);
            }
            b.off.push_back(b.ids.size());
        }
        if (hostile && !b.dense && b.n_docs && rnd(2)) {   // offsets that decrease or leave the token list, or tokens outside every document
            const u64 d = rnd(b.n_docs + 1), how = rnd(3);
            if (how == 0) b.off[d] = b.ids.size() + 1 + rnd(5);
            else if (how == 1) b.off[d] = b.off[d] > 0 ? b.off[d] - 1 - rnd(b.off[d]) : 0;
            else { const u64 cut = rnd(3); for (auto &o : b.off) o = o > cut ? o - cut : 0; }
        }
        const Result got = decode_by_lanes(t, b), want = decode_in_order(t, b);
        if (!(got == want)) {
            std::printf("round %ld: the lanes and the restatement differ (status %d/%d, where %llu/%llu, %zu/%zu bytes)\n", round, got.status, want.status, got.where,
                        want.where, got.out.size(), want.out.size());
            return 1;
        }
        bytes += got.out.size();
        errors += got.status != 0;
    }
    if (rounds >= 1000 && (!errors || !g_unstaged_tiles)) { std::printf("the rounds met %llu errors and %llu tiles beyond the stage\n", errors, g_unstaged_tiles); return 1; }
    std::printf("OK %ld rounds, %llu bytes, %llu refused, %llu tiles beyond the stage\n", rounds, bytes, errors, g_unstaged_tiles);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "batch")) return run_batch(argv[2]);
    if (argc == 4 && !std::strcmp(argv[1], "random")) return run_random(std::atol(argv[2]), std::strtoul(argv[3], nullptr, 10));
    std::fprintf(stderr, "usage: decode_check batch FILE | decode_check random ROUNDS SEED\n");
    return 2;
}
