// Host-only check of split_batch's per-position functions (no GPU needed): split_kernels.hip is compiled as plain C++
// (DAAC_SPLIT_HOST) and split_reach + split_start are evaluated at every position of random batches — documents of 0 .. 40 bytes over an
// alphabet of contraction letters, ', space, newline, letters, digits, punctuation, multi-byte characters of every class and malformed
// UTF-8, a batch with offsets[0] > 0 among them — against a sequential scanner of the definition that shares no code with them: units by
// Unicode Table 3-7, the pattern's alternatives tried in order, greedy, the fifth one backtracking.  Every document is handed over in a
// buffer of exactly its size and the mark bits in an array of exactly theirs, so built with -fsanitize=address,undefined a read outside
// the document ends the program.
//   usage: split_check [rounds] [seed]
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

// the classes from U+0080 on that the check runs with
struct Range { uint32_t first, last, cls; };
const Range kRanges[] = {{0x85, 0x85, 3},  {0xA0, 0xA0, 3},     {0xB2, 0xB3, 2},      {0xC0, 0xFF, 1},      {0x660, 0x669, 2},
                         {0x3000, 0x3000, 3}, {0x4E00, 0x9FFF, 1}, {0x10000, 0x1000B, 1}, {0x1D7CE, 0x1D7FF, 2}, {0x10FFFF, 0x10FFFF, 1}};

uint32_t class_of_cp(uint32_t cp) {
    if (cp < 0x80) {
        if ((cp >= 'A' && cp <= 'Z') || (cp >= 'a' && cp <= 'z')) return 1;
        if (cp >= '0' && cp <= '9') return 2;
        if (cp == 0x20 || (cp >= 0x09 && cp <= 0x0D)) return 3;
        return 0;
    }
    for (const Range &r : kRanges)
        if (cp >= r.first && cp <= r.last) return r.cls;
    return 0;
}

struct Unit { size_t at, len; uint32_t cls; };

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
        if (n) u.push_back(Unit{i, n, class_of_cp(cp)});
        else u.push_back(Unit{i, 1, static_cast<uint8_t>(d[i]) < 0x80 ? class_of_cp(static_cast<uint8_t>(d[i])) : 0u});
        i += n ? n : 1;
    }
    return u;
}

// the sequential scanner: the byte positions at which the words of d start
std::vector<size_t> scan(const std::string &d, int rule) {
    const std::vector<Unit> u = units_of(d);
    const size_t n = u.size();
    std::vector<size_t> starts;
    auto is = [&](size_t i, char c) { return i < n && u[i].len == 1 && d[u[i].at] == c; };
    auto run = [&](size_t i, auto pred) { while (i < n && pred(u[i])) ++i; return i; };
    for (size_t i = 0; i < n;) {
        starts.push_back(u[i].at);
        size_t e = i;
        if (rule == DAAC_SPLIT_WHITESPACE) {
            if (u[i].cls == 3) e = run(i, [](const Unit &x) { return x.cls == 3; });
            else e = run(i, [](const Unit &x) { return x.cls != 3; });
            i = e;
            continue;
        }
        // 's|'t|'re|'ve|'m|'ll|'d
        if (is(i, '\'')) {
            if (is(i + 1, 's') || is(i + 1, 't')) e = i + 2;
            else if (is(i + 1, 'r') && is(i + 2, 'e')) e = i + 3;
            else if (is(i + 1, 'v') && is(i + 2, 'e')) e = i + 3;
            else if (is(i + 1, 'm')) e = i + 2;
            else if (is(i + 1, 'l') && is(i + 2, 'l')) e = i + 3;
            else if (is(i + 1, 'd')) e = i + 2;
        }
        if (e == i) {   //  ?\p{L}+ |  ?\p{N}+ |  ?[^\s\p{L}\p{N}]+ : the optional space is taken first, then given back
            for (uint32_t cls : {1u, 2u, 0u}) {
                for (int space = 1; space >= 0 && e == i; --space) {
                    if (space && !is(i, ' ')) continue;
                    const size_t from = i + static_cast<size_t>(space);
                    const size_t to = run(from, [cls](const Unit &x) { return x.cls == cls; });
                    if (to > from) e = to;
                }
                if (e != i) break;
            }
        }
        if (e == i && u[i].cls == 3) {   // \s+(?!\S): the longest run, then shorter ones, that no non-whitespace unit follows
            const size_t full = run(i, [](const Unit &x) { return x.cls == 3; });
            for (size_t to = full; to > i && e == i; --to)
                if (to == n || u[to].cls == 3) e = to;
            if (e == i) e = full;        // \s+
        }
        if (e == i) { std::printf("MISMATCH the scanner matched nothing at unit %zu\n", i); std::exit(1); }
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

}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261018ull);
    auto below = [&](uint64_t n) { return static_cast<size_t>(rng() % n); };

    // the two-stage table, built here entry by entry (not the library's builder): exactly kSplitStage1 entries and the blocks in use
    std::vector<uint16_t> stage1(daac::kSplitStage1, 0);
    std::vector<uint8_t> stage2(daac::kSplitBlockBytes, 0);
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
    const daac::SplitTable tab{stage1.data(), stage2.data()};

    std::vector<std::string> alphabet = {"'", "'", "s", "t", "r", "e", "v", "m", "l", "l", "d", " ", " ", "\n", "\t", "a", "Z", "7", "0", "!", "-",
                                         "\x80", "\xC3", "\xE6\xBC", "\xED\xA0\x80", "\xF4\x90\x80\x80", "\xC0\xAF", "\xE0\x80\xAF", "\xF0\x9F", "\xFF", "\xBF"};
    for (uint32_t cp : {0xE9u, 0x6F22u, 0x663u, 0xB2u, 0x85u, 0xA0u, 0x3000u, 0x10000u, 0x1D7D0u, 0x10FFFFu, 0x1F600u, 0x2014u}) {
        alphabet.emplace_back();
        utf8(alphabet.back(), cp);
    }

    uint64_t n_docs = 0, n_words = 0;
    for (int round = 0; round < rounds; ++round) {
        // a batch: documents of 0 .. 40 bytes, cut anywhere (also inside a character), in front of them `front` bytes of no document
        const size_t nd = 1 + below(6), front = round % 3 == 0 ? 1 + below(5) : 0;
        std::vector<std::string> docs(nd);
        for (std::string &d : docs) {
            const size_t want = below(41);
            while (d.size() < want) d += alphabet[below(alphabet.size())];
            d.resize(want);
        }
        std::vector<uint64_t> off{front};
        for (const std::string &d : docs) off.push_back(off.back() + d.size());
        const uint64_t total = off.back() - off.front();
        // the mark bits as the kernel lays them out: non-empty documents' first positions and `total`, in exactly total / 32 + 1 words
        std::vector<uint32_t> marks(total / 32 + 1, 0);
        for (size_t i = 0; i < nd; ++i)
            if (!docs[i].empty()) marks[(off[i] - front) >> 5] |= 1u << ((off[i] - front) & 31);
        marks[total >> 5] |= 1u << (total & 31);
        for (int rule : {DAAC_SPLIT_WHITESPACE, DAAC_SPLIT_GPT2}) {
            for (size_t i = 0; i < nd; ++i) {
                const std::string &d = docs[i];
                const std::vector<size_t> want = scan(d, rule);
                // the document alone, in a heap block of exactly its size
                std::unique_ptr<uint8_t[]> buf(new uint8_t[d.size() ? d.size() : 1]);
                std::memcpy(buf.get(), d.data(), d.size());
                std::vector<size_t> got;
                for (size_t q = 0; q < d.size(); ++q) {
                    const uint64_t p = off[i] - front + q;
                    uint32_t win = 0;   // bit k: the mark of position p - kSplitBack + k
                    for (int k = 0; k < daac::kSplitBack + daac::kSplitAhead; ++k) {
                        const int64_t at = static_cast<int64_t>(p) - daac::kSplitBack + k;
                        if (at >= 0 && static_cast<uint64_t>(at) <= total && (marks[static_cast<size_t>(at) >> 5] >> (at & 31) & 1u)) win |= 1u << k;
                    }
                    int before = -1, ahead = -1;
                    daac::split_reach(win, before, ahead);
                    const int b_want = static_cast<int>(q < static_cast<size_t>(daac::kSplitBack) ? q : daac::kSplitBack);
                    const int a_want = static_cast<int>(d.size() - q < static_cast<size_t>(daac::kSplitAhead) ? d.size() - q : daac::kSplitAhead);
                    if (before != b_want || ahead != a_want) {
                        std::printf("MISMATCH round %d doc %zu position %zu: reach %d %d, expected %d %d\n", round, i, q, before, ahead, b_want, a_want);
                        return 1;
                    }
                    if (daac::split_start(tab, buf.get() + q, before, ahead, rule)) got.push_back(q);
                }
                if (got != want) {
                    std::printf("MISMATCH round %d rule %d doc %zu (%zu bytes):", round, rule, i, d.size());
                    for (unsigned char c : d) std::printf(" %02x", c);
                    std::printf("\n  expected");
                    for (size_t s : want) std::printf(" %zu", s);
                    std::printf("\n  got     ");
                    for (size_t s : got) std::printf(" %zu", s);
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
