// Host-only check of DAAC_SPLIT_O200K (no GPU needed): split_kernels.hip is compiled as plain C++ (DAAC_SPLIT_HOST) and the rule's
// functions are evaluated at every position against a sequential scanner of the pattern that shares no code with them.
//   1. Every string of up to `max_len` (default 6) symbols over the alphabet a A U+4E2D U+0301 0 space \n \t ' ! / s S, each a document
//      in a buffer of exactly its size: o200k_info, o200k_fwd_of and o200k_back_of at every position, the states walked with o200k_apply
//      and o200k_back_apply, o200k_start at every position.
//   2. Random batches walked as the kernels walk them — the positions' functions composed inside words of 64 positions by the steps of
//      the wave scan (o200k_then, o200k_back_then), o200k_span_map and o200k_span_back per tile, the spans of tiles as the carry
//      workgroup's lanes take them (o200k_span_carries), the words' carries, o200k_start — with tiles of 64, 128 and 1024 positions.
//      Batches hold random documents of 0 .. 40 bytes and documents with runs several tiles long (caseless letters, upper letters,
//      marks, newlines, digits, whitespace) between short random stretches, over an alphabet with letters of every case class, the
//      contraction letters in both cases, U+017F, multi-byte characters of every class and malformed UTF-8; some batches have
//      offsets[0] > 0 and empty documents.  Every second round runs with a class table that has U+017F in no class.
// Every document is handed over in a buffer of exactly its size, so built with -fsanitize=address,undefined a read outside the document
// ends the program.
//   usage: split_o200k_check [rounds] [seed] [max_len]
// prints "OK <rounds> rounds <strings> strings <docs> docs <words> words" or "MISMATCH ..." (exit status 1).
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
const Range kRanges[] = {{0x85, 0x85, 3},     {0xA0, 0xA0, 3},     {0xB2, 0xB3, 2},     {0xC0, 0xDE, 4},      {0xDF, 0xFF, 5},     {0x17F, 0x17F, 5},
                         {0x1C5, 0x1C5, 4},   {0x2B0, 0x2B0, 1},   {0x300, 0x36F, 6},   {0x660, 0x669, 2},    {0x2028, 0x2028, 3}, {0x3000, 0x3000, 3},
                         {0x4E00, 0x9FFF, 1}, {0x1D7CE, 0x1D7FF, 2}, {0x10FFFF, 0x10FFFF, 1}};
bool g_long_s = true;   // whether U+017F is a letter in this round's table
enum : uint32_t { O = 0, C = 1, N = 2, S = 3, UP = 4, LOW = 5, MARK = 6 };

uint32_t class_of_cp(uint32_t cp) {
    if (cp < 0x80) {
        if (cp >= 'A' && cp <= 'Z') return UP;
        if (cp >= 'a' && cp <= 'z') return LOW;
        if (cp >= '0' && cp <= '9') return N;
        if (cp == 0x20 || (cp >= 0x09 && cp <= 0x0D)) return S;
        return O;
    }
    if (cp == 0x17F && !g_long_s) return O;
    for (const Range &r : kRanges)
        if (cp >= r.first && cp <= r.last) return r.cls;
    return O;
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

void units_of(const std::string &d, std::vector<Unit> &u) {
    u.clear();
    for (size_t i = 0; i < d.size();) {
        uint32_t cp = 0;
        const size_t n = well_formed(d, i, cp);
        const uint32_t b = static_cast<uint8_t>(d[i]);
        if (n) u.push_back(Unit{i, n, class_of_cp(cp), cp});
        else u.push_back(Unit{i, 1, b < 0x80 ? class_of_cp(b) : 0u, b < 0x80 ? b : 0xFFFFFFFFu});
        i += n ? n : 1;
    }
}

// the sequential scanner: the byte positions at which the words of d start.  At each unit it tries the pattern's alternatives in order.
void scan(const std::string &d, std::vector<size_t> &starts) {
    static std::vector<Unit> u;
    units_of(d, u);
    const size_t n = u.size();
    starts.clear();
    auto fold = [&](size_t i) -> char {   // the letter unit i folds to, 0 if none
        if (i >= n) return 0;
        const uint32_t cp = u[i].cp;
        if (cp >= 'a' && cp <= 'z') return static_cast<char>(cp);
        if (cp >= 'A' && cp <= 'Z') return static_cast<char>(cp - 'A' + 'a');
        return cp == 0x17F && u[i].cls != O ? 's' : 0;
    };
    auto nl = [&](size_t i) { return u[i].cp == 0x0A || u[i].cp == 0x0D; };
    auto upper_side = [&](size_t i) { return u[i].cls == UP || u[i].cls == C || u[i].cls == MARK; };
    auto lower_side = [&](size_t i) { return u[i].cls == LOW || u[i].cls == C || u[i].cls == MARK; };
    auto suffix = [&](size_t e) {   // (?i:'s|'t|'re|'ve|'m|'ll|'d)?
        if (e < n && u[e].cp == '\'') {
            const char a = fold(e + 1), b = fold(e + 2);
            if (a == 's' || a == 't' || a == 'm' || a == 'd') return e + 2;
            if ((a == 'r' && b == 'e') || (a == 'v' && b == 'e') || (a == 'l' && b == 'l')) return e + 3;
        }
        return e;
    };
    auto word = [&](size_t i, bool first) {   // alternative 1 (U* Lw+) or 2 (U+ Lw*): the optional prefix is taken, then given back
        const bool prefix = u[i].cls != UP && u[i].cls != LOW && u[i].cls != C && u[i].cls != N && !nl(i);
        for (int with = prefix ? 1 : 0; with >= 0; --with) {
            const size_t start = i + static_cast<size_t>(with);
            size_t top = start;
            while (top < n && upper_side(top)) ++top;
            if (first) {
                for (size_t u_end = top + 1; u_end-- > start;) {   // the upper side gives back one unit at a time
                    size_t to = u_end;
                    while (to < n && lower_side(to)) ++to;
                    if (to > u_end) return suffix(to);
                }
            } else if (top > start) {
                size_t to = top;
                while (to < n && lower_side(to)) ++to;
                return suffix(to);
            }
        }
        return i;
    };
    for (size_t i = 0; i < n;) {
        starts.push_back(u[i].at);
        size_t e = word(i, true);
        if (e == i) e = word(i, false);
        if (e == i && u[i].cls == N) {   // \p{N}{1,3}
            while (e < n && e < i + 3 && u[e].cls == N) ++e;
        }
        if (e == i) {                    //  ?[^\s\p{L}\p{N}]+[\r\n/]*
            for (int space = 1; space >= 0 && e == i; --space) {
                if (space && u[i].cp != ' ') continue;
                const size_t from = i + static_cast<size_t>(space);
                size_t to = from;
                while (to < n && (u[to].cls == O || u[to].cls == MARK)) ++to;
                if (to > from) {
                    while (to < n && (nl(to) || u[to].cp == '/')) ++to;
                    e = to;
                }
            }
        }
        if (e == i) {                    // the whitespace alternatives
            if (u[i].cls != S) { std::printf("MISMATCH the scanner matched nothing at unit %zu\n", i); std::exit(1); }
            size_t full = i;
            while (full < n && u[full].cls == S) ++full;
            size_t last_nl = n;
            for (size_t k = i; k < full; ++k)
                if (nl(k)) last_nl = k;
            if (last_nl != n) e = last_nl + 1;                   // \s*[\r\n]+
            else if (full == n || full - 1 == i) e = full;       // \s+(?!\S) at the end, \s+
            else e = full - 1;                                   // \s+(?!\S)
        }
        i = e;
    }
}

void utf8(std::string &s, uint32_t cp) {
    if (cp < 0x80) s.push_back(static_cast<char>(cp));
    else if (cp < 0x800) { s.push_back(static_cast<char>(0xC0 | cp >> 6)); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else if (cp < 0x10000) { s.push_back(static_cast<char>(0xE0 | cp >> 12)); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else { s.push_back(static_cast<char>(0xF0 | cp >> 18)); s.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3F))); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
}
std::string utf8(uint32_t cp) { std::string s; utf8(s, cp); return s; }

struct Table {   // four bits a code point, as daac_splitter_create lays it out
    std::vector<uint16_t> stage1;
    std::vector<uint8_t> stage2;
    Table() : stage1(daac::kSplitStage1, 0), stage2(daac::kSplitBlockBytes4, 0) {
        for (uint32_t hi = 0; hi < daac::kSplitStage1; ++hi) {
            std::vector<uint8_t> blk(daac::kSplitBlockBytes4, 0);
            bool any = false;
            for (uint32_t lo = 0; lo < 256; ++lo) {
                const uint32_t cp = hi << 8 | lo, c = cp < 0x80 ? 0u : class_of_cp(cp);
                if (c) { any = true; blk[lo >> 1] = static_cast<uint8_t>(blk[lo >> 1] | c << (4 * (lo & 1))); }
            }
            if (!any) continue;
            stage1[hi] = static_cast<uint16_t>(stage2.size() / daac::kSplitBlockBytes4);
            stage2.insert(stage2.end(), blk.begin(), blk.end());
        }
    }
};

void report(const char *what, const std::string &d, const std::vector<size_t> &want, const std::vector<size_t> &got) {
    std::printf("MISMATCH %s (%zu bytes):", what, d.size());
    for (size_t k = 0; k < d.size() && k < 200; ++k) std::printf(" %02x", static_cast<unsigned char>(d[k]));
    std::printf("\n  expected");
    for (size_t k = 0; k < want.size() && k < 100; ++k) std::printf(" %zu", want[k]);
    std::printf("\n  got     ");
    for (size_t k = 0; k < got.size() && k < 100; ++k) std::printf(" %zu", got[k]);
    std::printf("\n");
}

// part 1: one document, the states walked position by position
bool check_string(const daac::SplitTable &tab, const std::string &d) {
    static std::vector<size_t> want, got;
    static std::vector<uint32_t> info, fwd_state, back_state;
    const size_t n = d.size();
    scan(d, want);
    got.clear();
    if (n == 0) return want.empty();
    std::unique_ptr<uint8_t[]> buf(new uint8_t[n]);
    std::memcpy(buf.get(), d.data(), n);
    info.assign(n, 0); fwd_state.assign(n, 0); back_state.assign(n, 0);
    auto reach = [&](size_t p, int &before, int &ahead) {
        before = p < static_cast<size_t>(daac::kSplitBack) ? static_cast<int>(p) : daac::kSplitBack;
        ahead = n - p < static_cast<size_t>(daac::kSplitAhead) ? static_cast<int>(n - p) : daac::kSplitAhead;
    };
    uint32_t st = daac::kQNone;
    for (size_t p = 0; p < n; ++p) {
        int before, ahead;
        reach(p, before, ahead);
        info[p] = daac::o200k_info(tab, buf.get() + p, before, ahead);
        fwd_state[p] = st;
        st = daac::o200k_apply(daac::o200k_fwd_of(info[p], p == 0), st);
    }
    uint32_t bs = 0;
    for (size_t p = n; p-- > 0;) {
        bs = daac::o200k_back_apply(daac::o200k_back_of(info[p], p + 1 == n), bs);
        back_state[p] = bs;
    }
    for (size_t p = 0; p < n; ++p) {
        int before, ahead;
        reach(p, before, ahead);
        if (daac::o200k_start(tab, buf.get() + p, before, ahead, info[p], fwd_state[p], back_state[p])) got.push_back(p);
    }
    if (got == want) return true;
    report("string", d, want, got);
    return false;
}

}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 1200;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261019ull);
    const int max_len = argc > 3 ? std::atoi(argv[3]) : 6;
    auto below = [&](uint64_t n) { return static_cast<size_t>(rng() % n); };

    g_long_s = true;
    const Table with_s;
    g_long_s = false;
    const Table without_s;

    // part 1
    uint64_t n_strings = 0;
    {
        g_long_s = true;
        const daac::SplitTable tab{with_s.stage1.data(), with_s.stage2.data()};
        const std::vector<std::string> small = {"a", "A", utf8(0x4E2D), utf8(0x301), "0", " ", "\n", "\t", "'", "!", "/", "s", "S"};
        std::vector<size_t> idx;
        std::string d;
        for (int len = 0; len <= max_len; ++len) {
            idx.assign(static_cast<size_t>(len), 0);
            for (;;) {
                d.clear();
                for (size_t k : idx) d += small[k];
                if (!check_string(tab, d)) return 1;
                ++n_strings;
                int k = len - 1;
                while (k >= 0 && ++idx[static_cast<size_t>(k)] == small.size()) idx[static_cast<size_t>(k--)] = 0;
                if (k < 0) break;
            }
        }
    }

    // part 2
    std::vector<std::string> alphabet = {"'", "'", "'", "s", "S", "t", "T", "r", "R", "e", "E", "v", "V", "m", "M", "l", "L", "l", "d", "D", " ", " ", " ", "\n", "\n", "\r", "\t",
                                         "a", "A", "B", "7", "0", "1", "!", "-", "/", "/", "\x80", "\xC5", "\xBF", "\xCC", "\xE6\xBC", "\xED\xA0\x80", "\xF4\x90\x80\x80", "\xC0\xAF", "\xF0\x9F",
                                         "\xFF"};
    for (uint32_t cp : {0xE9u, 0xC9u, 0x1C5u, 0x2B0u, 0x4E2Du, 0x4E2Du, 0x301u, 0x301u, 0x301u, 0x663u, 0xB2u, 0x85u, 0xA0u, 0x2028u, 0x3000u, 0x17Fu, 0x17Fu, 0x212Au, 0x1D7D0u,
                        0x10FFFFu, 0x1F600u, 0x2014u})
        alphabet.push_back(utf8(cp));
    const std::vector<std::string> run_pieces = {"1", utf8(0x663), " ", "\n", "\t", "\r", "\xC2\x85", utf8(0x4E2D), utf8(0x301), "A", utf8(0xC9), "/", "!", "a", utf8(0x2B0)};

    uint64_t n_docs = 0, n_words = 0;
    std::vector<size_t> want, got;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t tile = round % 16 == 15 ? 1024u : round % 2 ? 128u : 64u, words = tile / 64;
        const size_t carry_lanes = 1 + below(5);
        g_long_s = round % 2 == 0;
        const Table &table = g_long_s ? with_s : without_s;
        const daac::SplitTable tab{table.stage1.data(), table.stage2.data()};
        // a batch: documents cut anywhere (also inside a character), some empty, in front of them `front` bytes of no document
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
            } else if (below(8)) {
                const size_t want_len = below(41);
                while (d.size() < want_len) d += alphabet[below(alphabet.size())];
                d.resize(want_len);
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

        // pass 1: the functions of every position, the wave scans of every word, the functions of every tile
        const uint64_t n_pos = tiles * tile;
        std::vector<uint32_t> info(n_pos, 0), back(n_pos, daac::kBackIdentity), wback(tiles * words), tile_back(tiles), carry_f(tiles, 99), carry_b(tiles, 99);
        std::vector<unsigned long long> incl(n_pos, daac::kO200kIdentity), ex(n_pos), wmap(tiles * words), tile_map(tiles);
        for (uint64_t p = 0; p < total; ++p) {
            int before, ahead;
            reach(p, before, ahead);
            info[p] = daac::o200k_info(tab, byte_at(p), before, ahead);
            incl[p] = daac::o200k_fwd_of(info[p], mark_at(static_cast<int64_t>(p)));
            back[p] = daac::o200k_back_of(info[p], mark_at(static_cast<int64_t>(p) + 1));
        }
        for (uint64_t w = 0; w < tiles * words; ++w) {
            unsigned long long *m = incl.data() + w * 64;
            uint32_t *b = back.data() + w * 64;
            for (uint32_t d = 1; d < 64; d <<= 1) {   // the steps of the wave's scans, every lane from the values of the step before
                unsigned long long mo[64];
                uint32_t bo[64];
                std::memcpy(mo, m, sizeof(mo));
                std::memcpy(bo, b, sizeof(bo));
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    if (lane >= d) m[lane] = daac::o200k_then(mo[lane - d], mo[lane]);
                    if (lane + d < 64) b[lane] = daac::o200k_back_then(bo[lane + d], bo[lane]);
                }
            }
            for (uint32_t lane = 0; lane < 64; ++lane) ex[w * 64 + lane] = lane ? m[lane - 1] : daac::kO200kIdentity;
            wmap[w] = m[63];
            wback[w] = b[0];
        }
        for (uint64_t t = 0; t < tiles; ++t) {
            tile_map[t] = daac::o200k_span_map(wmap.data(), t * words, (t + 1) * words);
            tile_back[t] = daac::o200k_span_back(wback.data(), t * words, (t + 1) * words);
        }
        // pass 2: a lane per span of tiles, the spans' carries, then the tiles' carries
        {
            const uint64_t chunk = (tiles + carry_lanes - 1) / carry_lanes;
            std::vector<unsigned long long> s_map(carry_lanes);
            std::vector<uint32_t> s_back(carry_lanes), s_f(carry_lanes), s_b(carry_lanes);
            auto span = [&](size_t lane, uint64_t &begin, uint64_t &end) {
                begin = lane * chunk < tiles ? lane * chunk : tiles;
                end = begin + chunk < tiles ? begin + chunk : tiles;
            };
            uint64_t begin, end;
            for (size_t lane = 0; lane < carry_lanes; ++lane) {
                span(lane, begin, end);
                s_map[lane] = daac::o200k_span_map(tile_map.data(), begin, end);
                s_back[lane] = daac::o200k_span_back(tile_back.data(), begin, end);
            }
            daac::o200k_span_carries(s_map.data(), s_back.data(), 0, carry_lanes, daac::kQNone, 0u, s_f.data(), s_b.data());
            for (size_t lane = 0; lane < carry_lanes; ++lane) {
                span(lane, begin, end);
                daac::o200k_span_carries(tile_map.data(), tile_back.data(), begin, end, s_f[lane], s_b[lane], carry_f.data(), carry_b.data());
            }
        }
        // pass 3: the decision at every position
        std::vector<uint8_t> flag(total, 0);
        std::vector<uint32_t> cf(words), cb(words);
        for (uint64_t t = 0; t < tiles; ++t) {
            daac::o200k_span_carries(wmap.data() + t * words, wback.data() + t * words, 0, words, carry_f[t], carry_b[t], cf.data(), cb.data());
            for (uint32_t l = 0; l < tile && t * tile + l < total; ++l) {
                const uint64_t p = t * tile + l;
                int before, ahead;
                reach(p, before, ahead);
                flag[p] = daac::o200k_start(tab, byte_at(p), before, ahead, info[p], daac::o200k_apply(ex[p], cf[l >> 6]), daac::o200k_back_apply(back[p], cb[l >> 6]));
            }
        }
        for (size_t i = 0; i < nd; ++i) {
            const std::string &d = docs[i];
            scan(d, want);
            got.clear();
            for (size_t q = 0; q < d.size(); ++q)
                if (flag[off[i] - front + q]) got.push_back(q);
            if (got != want) {
                std::printf("round %d tile %u doc %zu at position %llu: ", round, tile, i, static_cast<unsigned long long>(off[i] - front));
                report("batch", d, want, got);
                return 1;
            }
            ++n_docs;
            n_words += want.size();
        }
    }
    std::printf("OK %d rounds %llu strings %llu docs %llu words\n", rounds, static_cast<unsigned long long>(n_strings), static_cast<unsigned long long>(n_docs),
                static_cast<unsigned long long>(n_words));
    return 0;
}
