// Host-only check of normalize_batch's per-position functions and of its two passes (no GPU needed): normalize_kernels.hip is compiled as
// plain C++ (DAAC_NORMALIZE_HOST).  Random batches — documents of 0 .. 40 bytes over an alphabet of ASCII, characters of every rule kind,
// characters of no rule and ill-formed UTF-8, cut anywhere, with offsets[0] > 0 — are normalized three ways and compared:
//   1. a sequential scanner of the definition that shares no code with the kernels' functions (Table 3-7 row by row, the rules searched
//      one by one);
//   2. norm_unit at every position of every document, the document alone in a heap block of exactly its size;
//   3. the two passes as the kernels run them, at tiles of 64, 128 and 1024 positions: the marks, a tile staged with kNormBack bytes in
//      front and kNormAhead - 1 behind (bytes outside the text are 0 and the text is a heap block of exactly its size), norm_window,
//      norm_reach and norm_unit per position, the tile sums, their exclusive sum, the ranks inside a tile, norm_store into a block of
//      exactly out_len bytes, src from the marks of the tile and norm_upper_bound, out_offsets from the marked positions and the pass
//      over the documents.
// norm_span_to_source is run on random spans of every normalized document, empty ones included, against the definition, and
// norm_unit_len against the splitter's split_unit_len on every window.  Built with -fsanitize=address,undefined, a read or a write
// outside a block ends the program.
//   usage: normalize_check [rounds] [seed]
// prints "OK <rounds> rounds <docs> docs <units> units <bytes> bytes out <spans> spans" or "MISMATCH ..." (exit status 1).
#define DAAC_NORMALIZE_HOST
#define DAAC_SPLIT_HOST
#include "../../daachorse_amd/csrc/normalize_kernels.hip"
#include "../../daachorse_amd/csrc/split_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

namespace {

struct Rule { uint32_t first, last, kind; std::string image; };
// sorted and disjoint; the images of the REPLACE rules go to the pool in this order
const std::vector<Rule> kRules = {
    {0x00, 0x00, daac::kNormDelete, ""}, {0x07, 0x07, daac::kNormDelete, ""}, {0x09, 0x0A, daac::kNormReplace, " "}, {'#', '#', daac::kNormPad, ""},
    {'A', 'A', daac::kNormReplace, "a"}, {'Q', 'Q', daac::kNormReplace, "quite a long image of a letter"}, {'Z', 'Z', daac::kNormReplace, "z"},
    {0x7F, 0x9F, daac::kNormDelete, ""}, {0xA0, 0xA0, daac::kNormReplace, " "}, {0xC9, 0xC9, daac::kNormReplace, "e"},
    {0x130, 0x130, daac::kNormReplace, "i\xCC\x87"}, {0x300, 0x36F, daac::kNormDelete, ""}, {0x391, 0x391, daac::kNormReplace, "\xCE\xB1"},
    {0x200D, 0x200D, daac::kNormDelete, ""}, {0x3000, 0x3000, daac::kNormReplace, " "}, {0x4E00, 0x9FFF, daac::kNormPad, ""},
    {0xAC00, 0xD7A3, daac::kNormHangul, ""}, {0xD800, 0xDFFF, daac::kNormDelete, ""}, {0xE000, 0xF8FF, daac::kNormDelete, ""},
    {0xF900, 0xF900, daac::kNormReplace, " \xE8\xB1\x88 "}, {0xFFFD, 0xFFFD, daac::kNormDelete, ""}, {0x1F600, 0x1F600, daac::kNormReplace, ":-)"},
    {0x20000, 0x2A6DF, daac::kNormPad, ""}, {0x10FFFF, 0x10FFFF, daac::kNormReplace, ""}};

// Table 3-7, row by row
size_t well_formed(const std::string &d, size_t i, uint32_t &cp) {
    auto b = [&](size_t k) { return static_cast<uint32_t>(static_cast<uint8_t>(d[k])); };
    auto in = [&](size_t k, uint32_t lo, uint32_t hi) { return k < d.size() && b(k) >= lo && b(k) <= hi; };
    const uint32_t b0 = b(i);
    if (b0 < 0x80) { cp = b0; return 1; }
    if (b0 >= 0xC2 && b0 <= 0xDF && in(i + 1, 0x80, 0xBF)) { cp = (b0 & 0x1F) << 6 | (b(i + 1) & 0x3F); return 2; }
    uint32_t lo = 0, hi = 0;
    if (b0 == 0xE0) { lo = 0xA0; hi = 0xBF; }
    else if ((b0 >= 0xE1 && b0 <= 0xEC) || b0 == 0xEE || b0 == 0xEF) { lo = 0x80; hi = 0xBF; }
    else if (b0 == 0xED) { lo = 0x80; hi = 0x9F; }
    if (hi && in(i + 1, lo, hi) && in(i + 2, 0x80, 0xBF)) { cp = (b0 & 0x0F) << 12 | (b(i + 1) & 0x3F) << 6 | (b(i + 2) & 0x3F); return 3; }
    lo = hi = 0;
    if (b0 == 0xF0) { lo = 0x90; hi = 0xBF; }
    else if (b0 >= 0xF1 && b0 <= 0xF3) { lo = 0x80; hi = 0xBF; }
    else if (b0 == 0xF4) { lo = 0x80; hi = 0x8F; }
    if (hi && in(i + 1, lo, hi) && in(i + 2, 0x80, 0xBF) && in(i + 3, 0x80, 0xBF)) {
        cp = (b0 & 0x07) << 18 | (b(i + 1) & 0x3F) << 12 | (b(i + 2) & 0x3F) << 6 | (b(i + 3) & 0x3F);
        return 4;
    }
    return 0;
}

void utf8(std::string &s, uint32_t cp) {
    if (cp < 0x80) s.push_back(static_cast<char>(cp));
    else if (cp < 0x800) { s.push_back(static_cast<char>(0xC0 | cp >> 6)); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else if (cp < 0x10000) { s.push_back(static_cast<char>(0xE0 | cp >> 12)); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else { s.push_back(static_cast<char>(0xF0 | cp >> 18)); s.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3F))); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
}

struct Unit { size_t at, len; };

// the sequential scanner: the image of d, per output byte the offset of its unit, and the units
void scan(const std::string &d, std::string &out, std::vector<uint32_t> &src, std::vector<Unit> &units) {
    out.clear();
    src.clear();
    units.clear();
    for (size_t i = 0; i < d.size();) {
        uint32_t cp = 0;
        const size_t n = well_formed(d, i, cp);
        const size_t len = n ? n : 1;
        std::string img = d.substr(i, len);
        if (n)
            for (const Rule &r : kRules)
                if (cp >= r.first && cp <= r.last) {
                    if (r.kind == daac::kNormDelete) img.clear();
                    else if (r.kind == daac::kNormReplace) img = r.image;
                    else if (r.kind == daac::kNormPad) img = " " + img + " ";
                    else {
                        const uint32_t s = cp - 0xAC00;
                        img.clear();
                        utf8(img, 0x1100 + s / 588);
                        utf8(img, 0x1161 + (s % 588) / 28);
                        if (s % 28) utf8(img, 0x11A7 + s % 28);
                    }
                }
        units.push_back(Unit{i, len});
        out += img;
        src.insert(src.end(), img.size(), static_cast<uint32_t>(i));
        i += len;
    }
}

template <class T>
std::unique_ptr<T[]> exact(const T *from, size_t n) {   // a heap block of exactly n elements
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    if (n && from) std::memcpy(p.get(), from, n * sizeof(T));
    else if (n) std::memset(p.get(), 0, n * sizeof(T));
    return p;
}

int fail(const char *what, int round, uint32_t tile) {
    std::printf("MISMATCH round %d tile %u: %s\n", round, tile, what);
    return 1;
}

}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261020ull);
    auto below = [&](uint64_t n) { return static_cast<size_t>(rng() % n); };

    // the table, built here entry by entry (not the library's builder): exactly the entries and the blocks in use
    std::string pool;
    std::vector<uint32_t> entry_of;
    for (const Rule &r : kRules) {
        uint32_t e = r.kind;
        if (r.kind == daac::kNormReplace) { e |= static_cast<uint32_t>(r.image.size()) << 3 | static_cast<uint32_t>(pool.size()) << 11; pool += r.image; }
        entry_of.push_back(e);
    }
    auto entry_at = [&](uint32_t cp) {
        for (size_t i = 0; i < kRules.size(); ++i)
            if (cp >= kRules[i].first && cp <= kRules[i].last) return entry_of[i];
        return 0u;
    };
    std::vector<uint32_t> ascii(128), stage2(daac::kNormBlock, 0);
    std::vector<uint16_t> stage1(daac::kNormStage1, 0);
    for (uint32_t cp = 0; cp < 128; ++cp) ascii[cp] = entry_at(cp);
    for (uint32_t hi = 0; hi < daac::kNormStage1; ++hi) {
        std::vector<uint32_t> blk(daac::kNormBlock, 0);
        bool any = false;
        for (uint32_t lo = 0; lo < 256; ++lo) any |= (blk[lo] = entry_at(hi << 8 | lo)) != 0;
        if (!any) continue;
        stage1[hi] = static_cast<uint16_t>(stage2.size() / daac::kNormBlock);
        stage2.insert(stage2.end(), blk.begin(), blk.end());
    }
    const auto pool_blk = exact(reinterpret_cast<const uint8_t *>(pool.data()), pool.size());
    const daac::NormTable tab{ascii.data(), stage1.data(), stage2.data(), pool_blk.get()};

    std::vector<std::string> alphabet = {"a", "b", "A", "Q", "Z", "#", " ", "\t", "\n", ".", std::string(1, '\0'), "\x07", "\x7F",
                                         "\x80", "\xC3", "\xE3\x80", "\xED\xA0\x80", "\xF4\x90\x80\x80", "\xC0\xAF", "\xF0\x9F", "\xFF", "\xBF", "\xEA\xB0"};
    for (uint32_t cp : {0xE9u, 0xC9u, 0x130u, 0x301u, 0x391u, 0x3B1u, 0xA0u, 0x200Du, 0x3000u, 0x4E2Du, 0x6F22u, 0xAC00u, 0xAC01u, 0xD55Cu, 0xD7A3u, 0xE000u, 0xF900u,
                        0xFFFDu, 0x1F600u, 0x1F601u, 0x20000u, 0x10FFFFu, 0x85u}) {
        alphabet.emplace_back();
        utf8(alphabet.back(), cp);
    }

    uint64_t n_docs = 0, n_units = 0, n_out = 0, n_spans = 0;
    for (int round = 0; round < rounds; ++round) {
        // ---- a batch
        const size_t nd = below(9), base = 1 + below(7);
        std::vector<std::string> docs(nd);
        std::vector<unsigned long long> off(nd + 1, base);
        std::string text;
        for (size_t i = 0; i < nd; ++i) {
            const size_t want_len = below(5) == 0 ? 0 : below(41);
            while (docs[i].size() < want_len) docs[i] += alphabet[below(alphabet.size())];
            docs[i].resize(want_len);   // cut anywhere, also inside a character
            text += docs[i];
            off[i + 1] = off[i] + want_len;
        }
        const uint64_t total = text.size();
        // ---- 1. the sequential scanner, and 2. norm_unit at every position of every document alone
        std::string want_out;
        std::vector<uint32_t> want_src;
        std::vector<unsigned long long> want_off(nd + 1, 0);
        std::vector<std::vector<Unit>> doc_units(nd);
        for (size_t i = 0; i < nd; ++i) {
            std::string o;
            std::vector<uint32_t> s;
            scan(docs[i], o, s, doc_units[i]);
            const auto buf = exact(reinterpret_cast<const uint8_t *>(docs[i].data()), docs[i].size());
            std::string got;
            size_t u = 0;
            for (size_t q = 0; q < docs[i].size(); ++q) {
                const int before = static_cast<int>(q < static_cast<size_t>(daac::kNormBack) ? q : daac::kNormBack);
                const int ahead = static_cast<int>(docs[i].size() - q < static_cast<size_t>(daac::kNormAhead) ? docs[i].size() - q : daac::kNormAhead);
                if (daac::norm_unit_len(buf.get() + q, ahead) != daac::split_unit_len(buf.get() + q, ahead)) return fail("norm_unit_len is not split_unit_len", round, 0);
                const daac::NormUnit nu = daac::norm_unit(tab, buf.get() + q, before, ahead);
                if (!nu.len) continue;
                if (u >= doc_units[i].size() || doc_units[i][u].at != q || doc_units[i][u].len != nu.len) return fail("norm_unit: the units", round, 0);
                ++u;
                const auto img = exact<uint8_t>(nullptr, nu.image);
                daac::norm_store(tab, nu, buf.get() + q, img.get());
                got.append(reinterpret_cast<const char *>(img.get()), nu.image);
            }
            if (u != doc_units[i].size() || got != o) return fail("norm_unit / norm_store: the image of a document", round, 0);
            want_out += o;
            want_src.insert(want_src.end(), s.begin(), s.end());
            want_off[i + 1] = want_out.size();
            n_units += doc_units[i].size();
        }
        n_docs += nd;
        n_out += want_out.size();
        if (nd == 0 || total == 0) continue;   // (the driver answers these without a launch)
        // ---- 3. the passes
        const auto txt = exact(reinterpret_cast<const uint8_t *>(text.data()), text.size());
        for (uint32_t tile_size : {64u, 128u, 1024u}) {
            const uint64_t tiles = (total + tile_size - 1) / tile_size;
            const uint32_t mark_words = tile_size / 32;
            const uint64_t n_mark = tiles * mark_words + 1;
            std::vector<uint32_t> marks_v(n_mark, 0);
            for (size_t d = 0; d <= nd; ++d) {   // the mark pass
                if (d < nd && off[d + 1] <= off[d]) continue;
                const uint64_t p = off[d] - base;
                marks_v[p >> 5] |= 1u << (p & 31);
            }
            const auto marks = exact(marks_v.data(), marks_v.size());
            std::vector<unsigned long long> counts(tiles, 0);
            std::vector<uint8_t> s_txt(tile_size + 16);
            std::vector<uint32_t> s_mark(mark_words + 2);
            auto stage = [&](uint64_t tile) {
                for (uint32_t i = 0; i < tile_size + daac::kNormBack + daac::kNormAhead - 1; ++i) {
                    const uint64_t p = tile * tile_size + i;
                    s_txt[i] = p >= static_cast<uint64_t>(daac::kNormBack) && p - daac::kNormBack < total ? txt[p - daac::kNormBack] : static_cast<uint8_t>(0);
                }
                for (uint32_t i = 0; i < mark_words + 2; ++i) {
                    const uint64_t w = tile * mark_words + i;
                    s_mark[i] = w >= 1 && w - 1 < n_mark ? marks[w - 1] : 0u;
                }
            };
            auto unit_at = [&](uint64_t tile, uint32_t l) {
                daac::NormUnit u{0, 0, 0, 0};
                if (tile * tile_size + l < total) {
                    int before, ahead;
                    daac::norm_reach(daac::norm_window(s_mark.data(), l + 32u - daac::kNormBack), before, ahead);
                    u = daac::norm_unit(tab, &s_txt[l + daac::kNormBack], before, ahead);
                }
                return u;
            };
            for (uint64_t tile = 0; tile < tiles; ++tile) {   // the count pass
                stage(tile);
                for (uint32_t l = 0; l < tile_size; ++l) counts[tile] += unit_at(tile, l).image;
            }
            unsigned long long out_len = 0;
            for (uint64_t tile = 0; tile < tiles; ++tile) { const unsigned long long c = counts[tile]; counts[tile] = out_len; out_len += c; }
            if (out_len != want_out.size()) return fail("the count pass: out_len", round, tile_size);
            const auto out = exact<uint8_t>(nullptr, out_len);
            const auto src = exact<uint32_t>(nullptr, out_len);
            std::vector<unsigned long long> out_off(nd + 1, ~0ull);
            for (uint64_t tile = 0; tile < tiles; ++tile) {   // the write pass
                stage(tile);
                const uint64_t tbase = tile * tile_size;
                std::vector<int32_t> last(mark_words);
                int32_t run = -1;
                for (uint32_t j = 0; j < mark_words; ++j) {
                    last[j] = run;
                    if (s_mark[1 + j]) run = static_cast<int32_t>(j * 32u + 31u - static_cast<uint32_t>(__builtin_clz(s_mark[1 + j])));
                }
                const unsigned long long doc0 = off[daac::norm_upper_bound(off.data(), nd + 1, base + tbase) - 1] - base;
                unsigned long long pos = counts[tile];
                for (uint32_t l = 0; l < tile_size; ++l) {
                    const uint64_t p = tbase + l;
                    const daac::NormUnit u = unit_at(tile, l);
                    const uint32_t m = s_mark[1 + (l >> 5)];
                    if (p < total && ((m >> (l & 31u)) & 1u)) {
                        const uint64_t d = daac::norm_upper_bound(off.data(), nd + 1, base + p) - 1;
                        if (d < nd) out_off[d] = pos;
                    }
                    if (u.image) {
                        if (pos + u.image > out_len) return fail("the write pass: a store beyond out_len", round, tile_size);
                        daac::norm_store(tab, u, &s_txt[l + daac::kNormBack], out.get() + pos);
                        const uint32_t at = m & (0xFFFFFFFFu >> (31u - (l & 31u)));
                        const unsigned long long first = at ? tbase + (l & ~31u) + 31u - static_cast<uint32_t>(__builtin_clz(at))
                                                             : last[l >> 5] >= 0 ? tbase + static_cast<uint32_t>(last[l >> 5]) : doc0;
                        for (uint32_t k = 0; k < u.image; ++k) src[pos + k] = static_cast<uint32_t>(p - first);
                    }
                    pos += u.image;
                }
            }
            for (size_t d = 0; d <= nd; ++d) {   // the pass over the documents
                if (off[d] >= base + total) { out_off[d] = out_len; continue; }
                if (d < nd && off[d + 1] > off[d]) continue;
                out_off[d] = out_off[daac::norm_upper_bound(off.data(), nd + 1, off[d]) - 1];
            }
            if (std::memcmp(out.get(), want_out.data(), out_len) != 0) return fail("the write pass: out", round, tile_size);
            if (out_len && std::memcmp(src.get(), want_src.data(), out_len * sizeof(uint32_t)) != 0) return fail("the write pass: src", round, tile_size);
            if (out_off != want_off) return fail("out_offsets", round, tile_size);
        }
        // ---- spans_to_source: two or three random spans a document, relative offsets over the text block
        std::vector<unsigned long long> rel(nd + 1), tok_off(nd + 1, 0), spans, want_spans;
        for (size_t d = 0; d <= nd; ++d) rel[d] = off[d] - base;
        for (size_t d = 0; d < nd; ++d) {
            const uint64_t ol = want_off[d + 1] - want_off[d], il = docs[d].size();
            for (size_t k = 0, nk = below(4); k < nk; ++k) {
                const uint64_t s = below(ol + 1), e = below(3) == 0 ? s : s + below(ol - s + 1);
                spans.push_back(s);
                spans.push_back(e);
                if (s == e) {
                    const uint64_t v = s < ol ? want_src[want_off[d] + s] : il;
                    want_spans.push_back(v);
                    want_spans.push_back(v);
                } else {
                    const uint64_t u = want_src[want_off[d] + e - 1];
                    size_t len = 0;
                    for (const Unit &x : doc_units[d]) if (x.at == u) len = x.len;
                    want_spans.push_back(want_src[want_off[d] + s]);
                    want_spans.push_back(u + len);
                }
            }
            tok_off[d + 1] = spans.size() / 2;
        }
        const auto sp = exact(spans.data(), spans.size());
        const auto src_blk = exact(want_src.data(), want_src.size());
        for (uint64_t t = 0; t < spans.size() / 2; ++t)
            daac::norm_span_to_source(sp.get() + 2 * t, t, tok_off.data(), want_off.data(), src_blk.get(), txt.get(), rel.data(), nd);
        if (!spans.empty() && std::memcmp(sp.get(), want_spans.data(), spans.size() * sizeof(unsigned long long)) != 0) return fail("spans_to_source", round, 0);
        n_spans += spans.size() / 2;
    }
    std::printf("OK %d rounds %llu docs %llu units %llu bytes out %llu spans\n", rounds, static_cast<unsigned long long>(n_docs), static_cast<unsigned long long>(n_units),
                static_cast<unsigned long long>(n_out), static_cast<unsigned long long>(n_spans));
    return 0;
}
