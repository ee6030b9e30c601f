// Host-only check of the scans and the decision of DAAC_SPLIT_CL100K and DAAC_SPLIT_LLAMA3 (no GPU needed): split_kernels.hip is compiled
// as plain C++ (DAAC_SPLIT_HOST) and the three passes are walked as the kernels walk them — split_pred at every position, the ballots
// gathered into split_planes, split_word_sum, split_span_sum per tile; split_span_sum and split_span_carries over spans of tiles as the
// carry workgroup's lanes take them; split_span_carries over a tile's words, split_scan_at and split_start_scanned at every position —
// with tiles of 64, 128 and 1024 positions, against a sequential scanner of the two patterns that shares no code with them.  Batches
// hold random documents of 0 .. 40 bytes and documents with runs of digits, whitespace and newlines several tiles long, over an alphabet
// with the contraction letters in both cases, U+017F, multi-byte characters of every class and malformed UTF-8; some batches have
// offsets[0] > 0.  Every document is handed over in a buffer of exactly its size, so built with -fsanitize=address,undefined a read
// outside the document ends the program.  Every second round runs with a class table that has U+017F in no class: it folds to s only as
// a letter.
//   usage: split_rules_check [rounds] [seed]
// prints "OK <rounds> rounds <docs> docs <words> words" or "MISMATCH ..." (exit status 1).
#define DAAC_SPLIT_HOST
#include "../../daachorse_amd/csrc/split_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

namespace {

struct Range { uint32_t first, last, cls; };
const Range kRanges[] = {{0x85, 0x85, 3},  {0xA0, 0xA0, 3},     {0xB2, 0xB3, 2},      {0xC0, 0xFF, 1},      {0x17F, 0x17F, 1},    {0x660, 0x669, 2},
                         {0x2028, 0x2028, 3}, {0x212A, 0x212A, 1}, {0x3000, 0x3000, 3}, {0x4E00, 0x9FFF, 1}, {0x1D7CE, 0x1D7FF, 2}, {0x10FFFF, 0x10FFFF, 1}};
bool g_long_s = true;   // whether U+017F is a letter in this round's table

uint32_t class_of_cp(uint32_t cp) {
    if (cp < 0x80) {
        if ((cp >= 'A' && cp <= 'Z') || (cp >= 'a' && cp <= 'z')) return 1;
        if (cp >= '0' && cp <= '9') return 2;
        if (cp == 0x20 || (cp >= 0x09 && cp <= 0x0D)) return 3;
        return 0;
    }
    if (cp == 0x17F && !g_long_s) return 0;
    for (const Range &r : kRanges)
        if (cp >= r.first && cp <= r.last) return r.cls;
    return 0;
}

struct Unit { size_t at, len; uint32_t cls, cp; };

// Table 3-7, row by row
size_t well_formed(const std::string &d, size_t i, uint32_t &cp) {
    auto b = [&](size_t k) { return static_cast<uint32_t>(static_cast<uint8_t>(d[k])); };
    auto in = [&](size_t k, uint32_t lo, uint32_t hi) { return k < d.size() && b(k) >= lo && b(k) <= hi; };
    const uint32_t b0 = b(i);
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

std::vector<Unit> units_of(const std::string &d) {
    std::vector<Unit> u;
    for (size_t i = 0; i < d.size();) {
        uint32_t cp = 0;
        const size_t n = well_formed(d, i, cp);
        const uint32_t b = static_cast<uint8_t>(d[i]);
        if (n) u.push_back(Unit{i, n, class_of_cp(cp), cp});
        else u.push_back(Unit{i, 1, b < 0x80 ? class_of_cp(b) : 0u, b < 0x80 ? b : 0xFFFFFFFFu});
        i += n ? n : 1;
    }
    return u;
}

// the sequential scanner: the byte positions at which the words of d start
std::vector<size_t> scan(const std::string &d, int rule) {
    const std::vector<Unit> u = units_of(d);
    const size_t n = u.size();
    std::vector<size_t> starts;
    auto fold = [&](size_t i) -> char {   // the letter unit i folds to, 0 if none
        if (i >= n) return 0;
        const uint32_t cp = u[i].cp;
        if (cp >= 'a' && cp <= 'z') return static_cast<char>(cp);
        if (cp >= 'A' && cp <= 'Z') return static_cast<char>(cp - 'A' + 'a');
        return cp == 0x17F && u[i].cls == 1 ? 's' : 0;
    };
    auto nl = [&](size_t i) { return u[i].cp == 0x0A || u[i].cp == 0x0D; };
    auto run_cls = [&](size_t i, uint32_t cls) { while (i < n && u[i].cls == cls) ++i; return i; };
    for (size_t i = 0; i < n;) {
        starts.push_back(u[i].at);
        size_t e = i;
        if (u[i].cp == '\'') {   // (?i:'s|'t|'re|'ve|'m|'ll|'d)
            const char a = fold(i + 1), b = fold(i + 2);
            if (a == 's' || a == 't' || a == 'm' || a == 'd') e = i + 2;
            else if ((a == 'r' && b == 'e') || (a == 'v' && b == 'e') || (a == 'l' && b == 'l')) e = i + 3;
        }
        if (e == i) {            // [^\r\n\p{L}\p{N}]?\p{L}+
            size_t first = n;
            if (u[i].cls == 1) first = i;
            else if (u[i].cls != 2 && !nl(i)) first = i + 1;
            const size_t to = run_cls(first, 1);
            if (to > first) e = to;
        }
        if (e == i && u[i].cls == 2) {   // \p{N}{1,3}
            e = run_cls(i, 2);
            if (e > i + 3) e = i + 3;
        }
        if (e == i) {            //  ?[^\s\p{L}\p{N}]+[\r\n]*
            for (int space = 1; space >= 0 && e == i; --space) {
                if (space && u[i].cp != ' ') continue;
                const size_t from = i + static_cast<size_t>(space);
                size_t to = run_cls(from, 0);
                if (to > from) {
                    while (to < n && nl(to)) ++to;
                    e = to;
                }
            }
        }
        if (e == i) {            // the whitespace alternatives
            if (u[i].cls != 3) { std::printf("MISMATCH the scanner matched nothing at unit %zu\n", i); std::exit(1); }
            const size_t full = run_cls(i, 3);
            size_t last_nl = n;
            for (size_t k = i; k < full; ++k)
                if (nl(k)) last_nl = k;
            if (rule == DAAC_SPLIT_CL100K && full == n) e = n;   // \s++$
            else if (last_nl != n) e = last_nl + 1;              // \s*[\r\n]+, \s*[\r\n]
            else if (full == n || full - 1 == i) e = full;       // \s+(?!\S) at the end, \s+
            else e = full - 1;                                   // \s+(?!\S)
        }
        i = e;
    }
    return starts;
}

void utf8(std::string &s, uint32_t cp) {
    if (cp < 0x80) s.push_back(static_cast<char>(cp));
    else if (cp < 0x800) { s.push_back(static_cast<char>(0xC0 | cp >> 6)); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else if (cp < 0x10000) { s.push_back(static_cast<char>(0xE0 | cp >> 12)); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else { s.push_back(static_cast<char>(0xF0 | cp >> 18)); s.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3F))); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
}

struct Table {
    std::vector<uint16_t> stage1;
    std::vector<uint8_t> stage2;
    Table() : stage1(daac::kSplitStage1, 0), stage2(daac::kSplitBlockBytes, 0) {
        for (uint32_t hi = 0; hi < daac::kSplitStage1; ++hi) {
            std::vector<uint8_t> blk(daac::kSplitBlockBytes, 0);
            bool any = false;
            for (uint32_t lo = 0; lo < 256; ++lo) {
                const uint32_t cp = hi << 8 | lo, c = cp < 0x80 ? 0u : class_of_cp(cp);
                if (c) { any = true; blk[lo >> 2] = static_cast<uint8_t>(blk[lo >> 2] | c << (2 * (lo & 3))); }
            }
            if (!any) continue;
            stage1[hi] = static_cast<uint16_t>(stage2.size() / daac::kSplitBlockBytes);
            stage2.insert(stage2.end(), blk.begin(), blk.end());
        }
    }
};

}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 1500;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261019ull);
    auto below = [&](uint64_t n) { return static_cast<size_t>(rng() % n); };

    g_long_s = true;
    const Table with_s;
    g_long_s = false;
    const Table without_s;

    std::vector<std::string> alphabet = {"'", "'", "'", "s", "S", "t", "T", "r", "R", "e", "E", "v", "V", "m", "M", "l", "L", "l", "d", "D", " ", " ", " ", "\n", "\n", "\r", "\t",
                                         "a", "7", "0", "1", "!", "-", "\x80", "\xC5", "\xBF", "\xE6\xBC", "\xED\xA0\x80", "\xF4\x90\x80\x80", "\xC0\xAF", "\xF0\x9F", "\xFF"};
    for (uint32_t cp : {0xE9u, 0x4E2Du, 0x663u, 0x663u, 0xB2u, 0x85u, 0xA0u, 0x2028u, 0x3000u, 0x17Fu, 0x17Fu, 0x212Au, 0x1D7D0u, 0x10FFFFu, 0x1F600u, 0x2014u}) {
        alphabet.emplace_back();
        utf8(alphabet.back(), cp);
    }
    std::string d2;   // the two-byte digit
    utf8(d2, 0x663);
    const std::vector<std::string> run_pieces = {"1", d2, " ", "\n", "\t", "\r", "\xC2\x85"};

    uint64_t n_docs = 0, n_words = 0;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t tile = round % 16 == 15 ? 1024u : round % 2 ? 128u : 64u, words = tile / 64;
        const size_t carry_lanes = 1 + below(5);
        g_long_s = round % 2 == 0;
        const Table &table = g_long_s ? with_s : without_s;
        const daac::SplitTable tab{table.stage1.data(), table.stage2.data()};
        // a batch: documents cut anywhere (also inside a character), in front of them `front` bytes of no document
        const size_t nd = 1 + below(8), front = round % 3 == 0 ? 1 + below(5) : 0;
        std::vector<std::string> docs(nd);
        for (std::string &d : docs) {
            if (below(4) == 0) {   // runs several tiles long, between short random stretches
                for (size_t part = 0, parts = 1 + below(3); part < parts; ++part) {
                    for (size_t k = below(6); k; --k) d += alphabet[below(alphabet.size())];
                    const std::string &a = run_pieces[below(run_pieces.size())], &b = below(3) ? a : run_pieces[below(run_pieces.size())];
                    const size_t len = below(3 * tile + 70), rare = 1 + below(len + 1);
                    for (size_t k = 0; k < len; ++k) d += k % rare == rare - 1 ? b : a;
                }
                for (size_t k = below(4); k; --k) d += alphabet[below(alphabet.size())];
                if (below(4) == 0) d.resize(below(d.size() + 1));
            } else {
                const size_t want = below(41);
                while (d.size() < want) d += alphabet[below(alphabet.size())];
                d.resize(want);
            }
        }
        std::vector<uint64_t> off{front};
        for (const std::string &d : docs) off.push_back(off.back() + d.size());
        const uint64_t total = off.back() - off.front();
        if (total == 0) continue;
        const uint64_t tiles = (total + tile - 1) / tile;
        // each document alone, in a heap block of exactly its size; the document of every position
        std::vector<std::unique_ptr<uint8_t[]>> bufs;
        std::vector<uint32_t> doc_of(total);
        for (size_t i = 0; i < nd; ++i) {
            bufs.emplace_back(new uint8_t[docs[i].size() ? docs[i].size() : 1]);
            std::memcpy(bufs.back().get(), docs[i].data(), docs[i].size());
            for (uint64_t p = off[i] - front; p < off[i + 1] - front; ++p) doc_of[p] = static_cast<uint32_t>(i);
        }
        // the mark bits as the kernel lays them out
        std::vector<uint32_t> marks(tiles * (tile / 32) + 1, 0);
        for (size_t i = 0; i < nd; ++i)
            if (!docs[i].empty()) marks[(off[i] - front) >> 5] |= 1u << ((off[i] - front) & 31);
        marks[total >> 5] |= 1u << (total & 31);
        auto mark_at = [&](int64_t at) { return at >= 0 && static_cast<uint64_t>(at) <= total && (marks[static_cast<size_t>(at) >> 5] >> (at & 31) & 1u); };
        auto reach = [&](uint64_t p, int &before, int &ahead) {
            uint32_t win = 0;   // bit k: the mark of position p - kSplitBack + k
            for (int k = 0; k < daac::kSplitBack + daac::kSplitAhead; ++k)
                if (mark_at(static_cast<int64_t>(p) - daac::kSplitBack + k)) win |= 1u << k;
            daac::split_reach(win, before, ahead);
        };
        auto byte_at = [&](uint64_t p) { return bufs[doc_of[p]].get() + (p - (off[doc_of[p]] - front)); };

        // pass 1: the masks and functions of every word, the function of every tile
        std::vector<daac::SplitPlanes> planes(tiles * words);
        std::vector<uint32_t> wsum(tiles * words), tile_sum(tiles), carry_f(tiles, 99), carry_b(tiles, 99);
        for (uint64_t w = 0; w < tiles * words; ++w) {
            uint64_t u = 0, n = 0, s = 0, nl = 0, o = 0, m0 = 0, m1 = 0;
            for (uint32_t k = 0; k < 64; ++k) {
                const uint64_t p = w * 64 + k;
                if (p >= total) break;
                int before, ahead;
                reach(p, before, ahead);
                const uint32_t bits = daac::split_pred(tab, byte_at(p), before, ahead);
                u |= static_cast<uint64_t>(bits & daac::kPredU ? 1 : 0) << k;
                n |= static_cast<uint64_t>(bits & daac::kPredN ? 1 : 0) << k;
                s |= static_cast<uint64_t>(bits & daac::kPredS ? 1 : 0) << k;
                nl |= static_cast<uint64_t>(bits & daac::kPredNl ? 1 : 0) << k;
                o |= static_cast<uint64_t>(bits & daac::kPredO ? 1 : 0) << k;
                m0 |= static_cast<uint64_t>(mark_at(static_cast<int64_t>(p)) ? 1 : 0) << k;
                m1 |= static_cast<uint64_t>(mark_at(static_cast<int64_t>(p) + 1) ? 1 : 0) << k;
            }
            planes[w] = daac::split_planes(u, n, s, nl, o, m0, m1);
            wsum[w] = daac::split_word_sum(planes[w]);
        }
        for (uint64_t t = 0; t < tiles; ++t) tile_sum[t] = daac::split_span_sum(wsum.data(), t * words, (t + 1) * words);
        // pass 2: a lane per span of tiles, the spans' carries, then the tiles' carries
        {
            const uint64_t chunk = (tiles + carry_lanes - 1) / carry_lanes;
            std::vector<uint32_t> s_sum(carry_lanes), s_f(carry_lanes), s_b(carry_lanes);
            auto span = [&](size_t lane, uint64_t &begin, uint64_t &end) {
                begin = lane * chunk < tiles ? lane * chunk : tiles;
                end = begin + chunk < tiles ? begin + chunk : tiles;
            };
            uint64_t begin, end;
            for (size_t lane = 0; lane < carry_lanes; ++lane) { span(lane, begin, end); s_sum[lane] = daac::split_span_sum(tile_sum.data(), begin, end); }
            daac::split_span_carries(s_sum.data(), 0, carry_lanes, 0u, 0u, s_f.data(), s_b.data());
            for (size_t lane = 0; lane < carry_lanes; ++lane) {
                span(lane, begin, end);
                daac::split_span_carries(tile_sum.data(), begin, end, s_f[lane], s_b[lane], carry_f.data(), carry_b.data());
            }
        }
        // pass 3: the decision at every position
        std::vector<uint8_t> flag(total, 0);
        for (int rule : {DAAC_SPLIT_CL100K, DAAC_SPLIT_LLAMA3}) {
            std::vector<uint32_t> cf(words), cb(words);
            for (uint64_t t = 0; t < tiles; ++t) {
                daac::split_span_carries(wsum.data() + t * words, 0, words, carry_f[t], carry_b[t], cf.data(), cb.data());
                for (uint32_t l = 0; l < tile && t * tile + l < total; ++l) {
                    const uint64_t p = t * tile + l;
                    int before, ahead;
                    reach(p, before, ahead);
                    const daac::SplitScan sc = daac::split_scan_at(planes[t * words + (l >> 6)], l & 63u, cf[l >> 6], cb[l >> 6]);
                    flag[p] = daac::split_start_scanned(tab, byte_at(p), before, ahead, rule, sc);
                }
            }
            for (size_t i = 0; i < nd; ++i) {
                const std::string &d = docs[i];
                const std::vector<size_t> want = scan(d, rule);
                std::vector<size_t> got;
                for (size_t q = 0; q < d.size(); ++q)
                    if (flag[off[i] - front + q]) got.push_back(q);
                if (got != want) {
                    std::printf("MISMATCH round %d rule %d tile %u doc %zu at position %llu (%zu bytes):", round, rule, tile, i, static_cast<unsigned long long>(off[i] - front), d.size());
                    for (size_t k = 0; k < d.size() && k < 200; ++k) std::printf(" %02x", static_cast<unsigned char>(d[k]));
                    std::printf("\n  expected");
                    for (size_t k = 0; k < want.size() && k < 100; ++k) std::printf(" %zu", want[k]);
                    std::printf("\n  got     ");
                    for (size_t k = 0; k < got.size() && k < 100; ++k) std::printf(" %zu", got[k]);
                    std::printf("\n");
                    return 1;
                }
                ++n_docs;
                n_words += want.size();
            }
        }
    }
    std::printf("OK %d rounds %llu docs %llu words\n", rounds, static_cast<unsigned long long>(n_docs), static_cast<unsigned long long>(n_words));
    return 0;
}
