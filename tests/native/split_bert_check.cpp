// Host-only check of the DAAC_SPLIT_BERT branch of split_start and of the words-space body (no GPU needed): split_kernels.hip is compiled
// as plain C++ (DAAC_SPLIT_HOST).  split_start is evaluated at every position of random documents — 0 .. 40 bytes over an alphabet of
// letters, digits, ASCII and multi-byte punctuation, whitespace of one, two and three bytes, symbols, a control character and malformed
// UTF-8, cut anywhere — against a sequential scanner of the definition that shares no code with it: a maximal run of S units is a word,
// every O unit is a word of its own, a maximal run of L and N units is a word.  split_word_space is evaluated on every word of that
// scan and on random byte ranges that begin or end inside a character, against the class of the range's first unit.  Every document and
// every range is handed over in a heap block of exactly its size, so built with -fsanitize=address,undefined a read outside it ends the
// program.
//   usage: split_bert_check [rounds] [seed]
// prints "OK <rounds> rounds <docs> docs <words> words <space> space" or "MISMATCH ..." (exit status 1).
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

// the classes from U+0080 on that the check runs with: punctuation (U+00BF, U+2014, U+3001) is in no range
struct Range { uint32_t first, last, cls; };
const Range kRanges[] = {{0x85, 0x85, 3}, {0xA0, 0xA0, 3}, {0xA2, 0xA5, 1}, {0xB2, 0xB3, 2}, {0xC0, 0xFF, 1}, {0x300, 0x36F, 1}, {0x660, 0x669, 2},
                         {0x3000, 0x3000, 3}, {0x4E00, 0x9FFF, 1}, {0x1F600, 0x1F64F, 1}, {0x10FFFF, 0x10FFFF, 1}};

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

// the sequential scanner: the byte positions at which the words of d start, and whether each word is whitespace
void scan(const std::string &d, std::vector<size_t> &starts, std::vector<uint8_t> &space) {
    const std::vector<Unit> u = units_of(d);
    starts.clear();
    space.clear();
    for (size_t i = 0; i < u.size();) {
        starts.push_back(u[i].at);
        space.push_back(u[i].cls == 3);
        size_t e = i + 1;
        if (u[i].cls == 3) while (e < u.size() && u[e].cls == 3) ++e;
        else if (u[i].cls != 0) while (e < u.size() && (u[e].cls == 1 || u[e].cls == 2)) ++e;
        i = e;
    }
}

void utf8(std::string &s, uint32_t cp) {
    if (cp < 0x80) s.push_back(static_cast<char>(cp));
    else if (cp < 0x800) { s.push_back(static_cast<char>(0xC0 | cp >> 6)); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else if (cp < 0x10000) { s.push_back(static_cast<char>(0xE0 | cp >> 12)); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
    else { s.push_back(static_cast<char>(0xF0 | cp >> 18)); s.push_back(static_cast<char>(0x80 | ((cp >> 12) & 0x3F))); s.push_back(static_cast<char>(0x80 | ((cp >> 6) & 0x3F))); s.push_back(static_cast<char>(0x80 | (cp & 0x3F))); }
}

// split_word_space on a heap block of exactly the range's size
uint8_t word_space(const daac::SplitTable &tab, const std::string &d, size_t s, size_t e) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[e > s ? e - s : 1]);
    std::memcpy(buf.get(), d.data() + s, e - s);
    return daac::split_word_space(tab, buf.get(), 0, e - s);
}

}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261019ull);
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

    std::vector<std::string> alphabet = {"a", "b", "Z", "7", "0", " ", " ", "\n", "\t", "!", ".", ",", "'", "-", "#", "$", "\x01", "\x7F",
                                         "\x80", "\xC3", "\xE3\x80", "\xED\xA0\x80", "\xF4\x90\x80\x80", "\xC0\xAF", "\xF0\x9F", "\xFF", "\xBF"};
    for (uint32_t cp : {0xE9u, 0x6F22u, 0x663u, 0xB2u, 0x85u, 0xA0u, 0x3000u, 0x3001u, 0x3001u, 0xBFu, 0x2014u, 0xA2u, 0x301u, 0x1F600u, 0x10FFFFu}) {
        alphabet.emplace_back();
        utf8(alphabet.back(), cp);
    }

    uint64_t n_docs = 0, n_words = 0, n_space = 0;
    for (int round = 0; round < rounds; ++round) {
        for (size_t i = 0, nd = 1 + below(6); i < nd; ++i) {
            std::string d;
            const size_t want_len = below(41);
            while (d.size() < want_len) d += alphabet[below(alphabet.size())];
            d.resize(want_len);   // cut anywhere, also inside a character
            std::vector<size_t> want, got;
            std::vector<uint8_t> want_space;
            scan(d, want, want_space);
            std::unique_ptr<uint8_t[]> buf(new uint8_t[d.size() ? d.size() : 1]);   // the document alone, in a heap block of exactly its size
            std::memcpy(buf.get(), d.data(), d.size());
            for (size_t q = 0; q < d.size(); ++q) {
                const int before = static_cast<int>(q < static_cast<size_t>(daac::kSplitBack) ? q : daac::kSplitBack);
                const int ahead = static_cast<int>(d.size() - q < static_cast<size_t>(daac::kSplitAhead) ? d.size() - q : daac::kSplitAhead);
                if (daac::split_start(tab, buf.get() + q, before, ahead, DAAC_SPLIT_BERT)) got.push_back(q);
            }
            if (got != want) {
                std::printf("MISMATCH round %d doc %zu (%zu bytes):", round, i, d.size());
                for (unsigned char c : d) std::printf(" %02x", c);
                std::printf("\n  expected");
                for (size_t s : want) std::printf(" %zu", s);
                std::printf("\n  got     ");
                for (size_t s : got) std::printf(" %zu", s);
                std::printf("\n");
                return 1;
            }
            for (size_t w = 0; w < want.size(); ++w) {
                const size_t s = want[w], e = w + 1 < want.size() ? want[w + 1] : d.size();
                if (word_space(tab, d, s, e) != want_space[w]) { std::printf("MISMATCH round %d doc %zu word %zu: words_space\n", round, i, w); return 1; }
                n_space += want_space[w];
            }
            for (int k = 0; k < 4; ++k) {   // any byte range: its first unit is taken inside the range
                const size_t s = below(d.size() + 1), e = s + below(d.size() - s + 1);
                const std::vector<Unit> u = units_of(d.substr(s, e - s));
                const uint8_t expect = !u.empty() && u[0].cls == 3;
                if (word_space(tab, d, s, e) != expect) { std::printf("MISMATCH round %d doc %zu range %zu..%zu: words_space\n", round, i, s, e); return 1; }
            }
            ++n_docs;
            n_words += want.size();
        }
    }
    std::printf("OK %d rounds %llu docs %llu words %llu space\n", rounds, static_cast<unsigned long long>(n_docs), static_cast<unsigned long long>(n_words),
                static_cast<unsigned long long>(n_space));
    return 0;
}
