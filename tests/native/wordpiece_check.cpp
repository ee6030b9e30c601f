// Host-only check of tokenize_wordpiece's per-lane bodies (no GPU needed): wordpiece_kernels.hip is compiled as plain C++
// (DAAC_WORDPIECE_HOST) and its count and write bodies are run document by document.  Every array has exactly the size the driver gives
// it, so built with -fsanitize=address,undefined a read or write outside it ends the program; a lane that writes a slot outside its own
// slice is reported too.
//   wordpiece_check words <file>      the pieces and words of <file> (written by the test from the fixtures): lines
//                                       M <unk_id> <max_chars>
//                                       P <hex of the piece> <first id> <continuation id>     (0xFFFFFFFF as 4294967295)
//                                       W <hex of the word, or - for the empty word>
//                                     all words are one batch; every occurrence of a piece is a tuple.  Prints per word one line of
//                                     id:start:end tokens.
//   wordpiece_check hostile [rounds] [seed]
//                                     random words, pieces with "" among them and roles that lack ids, skip flags, a character cap, and
//                                     tuple lists with hostile entries mixed in — ends beyond L, zero lengths, len > end, values beyond
//                                     the id tables — in sorted, reversed and shuffled order, and empty lists, against a restatement of
//                                     the definition that shares no code with the bodies.  Prints "OK <rounds> rounds .." or "MISMATCH ..".
#define DAAC_WORDPIECE_HOST
#include "../../daachorse_amd/csrc/wordpiece_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

namespace {

struct Tok { uint32_t id; uint64_t start, end; };
struct Piece { std::string bytes; uint32_t first, cont; };

std::string unhex(const std::string &h) {
    std::string out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back(static_cast<char>(std::stoi(h.substr(i, 2), nullptr, 16)));
    return out;
}

// one batch through the two bodies: docs behind `lead` bytes that belong to nobody, seg / first the tuple CSR
struct Batch {
    std::vector<std::string> docs;
    std::vector<daac::WpTuple> seg;
    std::vector<unsigned long long> first;   // docs + 1
    std::vector<uint8_t> skip;               // empty: none
    uint64_t lead = 0;
};

// -> false when a lane wrote outside its slice
bool run(const Batch &b, const std::vector<uint32_t> &first_ids, const std::vector<uint32_t> &cont_ids, uint32_t unk_id, uint32_t max_chars,
         std::vector<std::vector<Tok>> &out) {
    const uint64_t n = b.docs.size();
    std::vector<unsigned long long> off(n + 1, b.lead);
    std::vector<uint8_t> text;   // the documents only: a.hay is byte 0 of document 0
    for (uint64_t d = 0; d < n; ++d) {
        off[d + 1] = off[d] + b.docs[d].size();
        text.insert(text.end(), b.docs[d].begin(), b.docs[d].end());
    }
    const uint64_t len = off[n] - off[0], pos = len + n;
    const daac::WpSlot junk{0xDEADBEEFu, 0xDEADBEEFu};
    std::vector<daac::WpSlot> slots(pos, junk);
    std::vector<unsigned long long> tok_off(n + 1, ~0ull);
    daac::WpArgs a{};
    a.hay = text.data();
    a.seg = b.seg.data();
    a.doc_first = b.first.data();
    a.doc_off = off.data();
    a.n_docs = n;
    a.first_ids = first_ids.data();
    a.cont_ids = cont_ids.data();
    a.n_ids = first_ids.size();
    a.unk_id = unk_id;
    a.max_chars = max_chars;
    a.skip = b.skip.empty() ? nullptr : b.skip.data();
    a.slots = slots.data();
    a.tok_offsets = tok_off.data();
    for (uint64_t d = 0; d < n; ++d) {
        const std::vector<daac::WpSlot> before = slots;
        tok_off[d] = daac::wp_count_lane(a, d);
        const uint64_t lo = off[d] - off[0] + d, hi = lo + b.docs[d].size() + 1;   // the lane's slice
        for (uint64_t q = 0; q < pos; ++q)
            if ((q < lo || q >= hi) && std::memcmp(&before[q], &slots[q], sizeof(daac::WpSlot)) != 0) return false;
    }
    unsigned long long total = 0;
    for (uint64_t d = 0; d <= n; ++d) { const unsigned long long c = d < n ? tok_off[d] : 0; tok_off[d] = total; total += c; }
    std::vector<uint32_t> ids(total, 0xDEADBEEFu);
    std::vector<unsigned long long> spans(2 * total, ~0ull);
    a.ids = ids.data();
    a.spans = spans.data();
    for (uint64_t d = 0; d < n; ++d) daac::wp_write_lane(a, d);
    out.assign(n, {});
    for (uint64_t d = 0; d < n; ++d)
        for (unsigned long long x = tok_off[d]; x < tok_off[d + 1]; ++x) out[d].push_back(Tok{ids[x], spans[2 * x], spans[2 * x + 1]});
    return true;
}

// every occurrence of a piece in doc, by end
void occurrences(const std::string &doc, const std::vector<Piece> &pieces, bool reversed, std::vector<daac::WpTuple> &seg) {
    for (uint64_t e = 0; e <= doc.size(); ++e)
        for (size_t k = 0; k < pieces.size(); ++k) {
            const size_t i = reversed ? pieces.size() - 1 - k : k;
            const std::string &p = pieces[i].bytes;
            if (p.size() <= e && doc.compare(e - p.size(), p.size(), p) == 0) seg.push_back(daac::WpTuple{e, static_cast<uint32_t>(p.size()), static_cast<uint32_t>(i)});
        }
}

// the definition, for one document
std::vector<Tok> restate(const std::string &doc, const std::vector<Piece> &pieces, uint32_t unk_id, uint32_t max_chars) {
    std::vector<Tok> out;
    const size_t L = doc.size();
    if (!L) return out;
    size_t chars = 0;
    for (unsigned char c : doc) chars += (c & 0xC0) != 0x80;
    const std::vector<Tok> unk{Tok{unk_id, 0, L}};
    if (chars > max_chars) return unk;
    std::map<std::string, const Piece *> by;
    for (const Piece &p : pieces) by[p.bytes] = &p;
    for (size_t p = 0; p < L;) {
        size_t e = L;
        for (; e > p; --e) {
            const auto it = by.find(doc.substr(p, e - p));
            if (it == by.end()) continue;
            const uint32_t id = p ? it->second->cont : it->second->first;
            if (id == 0xFFFFFFFFu) continue;
            out.push_back(Tok{id, p, e});
            break;
        }
        if (e == p) return unk;
        p = e;
    }
    return out;
}

int words_mode(const char *path) {
    std::ifstream in(path);
    if (!in) { std::printf("cannot read %s\n", path); return 2; }
    std::vector<Piece> pieces;
    Batch b;
    uint32_t unk_id = 0, max_chars = 100;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind, hex;
        ls >> kind;
        if (kind == "M") ls >> unk_id >> max_chars;
        else if (kind == "P") { Piece p; ls >> hex >> p.first >> p.cont; p.bytes = unhex(hex); pieces.push_back(p); }
        else if (kind == "W") { ls >> hex; b.docs.push_back(unhex(hex)); }
    }
    // pieces by their bytes: a word's occurrences are looked up, not searched
    std::map<std::string, uint32_t> index;
    size_t longest = 0;
    for (size_t i = 0; i < pieces.size(); ++i) { index[pieces[i].bytes] = static_cast<uint32_t>(i); longest = std::max(longest, pieces[i].bytes.size()); }
    b.lead = 3;
    for (const std::string &doc : b.docs) {
        b.first.push_back(b.seg.size());
        for (uint64_t e = 0; e <= doc.size(); ++e)
            for (uint64_t l = std::min<uint64_t>(e, longest) + 1; l-- > 0;) {   // longest first at an end, as the scan reports them
                const auto it = index.find(doc.substr(e - l, l));
                if (it != index.end()) b.seg.push_back(daac::WpTuple{e, static_cast<uint32_t>(l), it->second});
            }
    }
    b.first.push_back(b.seg.size());
    std::vector<uint32_t> first_ids, cont_ids;
    for (const Piece &p : pieces) { first_ids.push_back(p.first); cont_ids.push_back(p.cont); }
    std::vector<std::vector<Tok>> got;
    if (!run(b, first_ids, cont_ids, unk_id, max_chars, got)) { std::printf("a lane wrote outside its slice\n"); return 1; }
    for (const std::vector<Tok> &toks : got) {
        std::string s;
        for (const Tok &t : toks) s += (s.empty() ? "" : " ") + std::to_string(t.id) + ":" + std::to_string(t.start) + ":" + std::to_string(t.end);
        std::printf("%s\n", s.c_str());
    }
    return 0;
}

int hostile_mode(int rounds, uint64_t seed) {
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return static_cast<uint64_t>(rng() % n); };
    const std::string alphabets[3] = {"ab", "abc", std::string("a\x80\xc3\xa9", 4)};
    uint64_t docs_total = 0, toks_total = 0, unk_total = 0, hostile_total = 0;
    for (int r = 0; r < rounds; ++r) {
        const std::string &alpha = alphabets[below(3)];
        std::vector<Piece> pieces;
        if (below(3) == 0) pieces.push_back(Piece{"", 900, 901});
        for (uint64_t i = 0, np = 1 + below(14); i < np; ++i) {
            Piece p;
            for (uint64_t j = 0, l = 1 + below(below(4) ? 3 : 6); j < l; ++j) p.bytes += alpha[below(alpha.size())];
            bool seen = false;
            for (const Piece &q : pieces) seen = seen || q.bytes == p.bytes;
            if (seen) continue;   // patterns are unique
            p.first = below(4) == 0 ? 0xFFFFFFFFu : static_cast<uint32_t>(100 + 2 * pieces.size());
            p.cont = below(4) == 0 ? 0xFFFFFFFFu : static_cast<uint32_t>(101 + 2 * pieces.size());
            pieces.push_back(p);
        }
        std::vector<uint32_t> first_ids, cont_ids;
        for (const Piece &p : pieces) { first_ids.push_back(p.first); cont_ids.push_back(p.cont); }
        const uint32_t unk_id = below(2) ? 7u : 0xFFFFFFFFu, max_chars = below(3) ? 0xFFFFFFFFu : static_cast<uint32_t>(1 + below(12));
        Batch b;
        b.lead = below(4);
        const uint64_t n = 1 + below(6), order = below(4);   // 0: by end; 1: by end, pieces reversed; 2: shuffled; 3: no tuples at all
        if (below(3) == 0) b.skip.assign(n, 0);
        for (uint64_t d = 0; d < n; ++d) {
            std::string doc;
            for (uint64_t j = 0, l = below(4) == 0 ? 0 : below(31); j < l; ++j) doc += alpha[below(alpha.size())];
            b.docs.push_back(doc);
            if (!b.skip.empty()) b.skip[d] = below(3) == 0 ? static_cast<uint8_t>(1 + below(255)) : 0;
            b.first.push_back(b.seg.size());
            if (order == 3) continue;
            const size_t from = b.seg.size();
            occurrences(doc, pieces, order == 1, b.seg);
            const uint64_t L = doc.size();
            for (uint64_t h = 0, nh = below(5); h < nh; ++h) {   // entries no scan produces: each is invalid in one way
                const uint32_t v = static_cast<uint32_t>(below(pieces.size()));
                daac::WpTuple t{};
                switch (below(5)) {
                    case 0: t = daac::WpTuple{L + 1 + below(5), static_cast<uint32_t>(1 + below(3)), v}; break;          // an end beyond L
                    case 1: t = daac::WpTuple{below(L + 1), 0u, v}; break;                                              // a zero length
                    case 2: { const uint64_t e = below(L + 1); t = daac::WpTuple{e, static_cast<uint32_t>(e + 1 + below(4)), v}; break; }   // len > end
                    case 3: t = daac::WpTuple{L ? 1 + below(L) : 0, 1u, static_cast<uint32_t>(pieces.size() + below(3))}; break;   // a value beyond the tables
                    default: t = daac::WpTuple{~0ull - below(3), 0xFFFFFFFFu, 0xFFFFFFFFu}; break;
                }
                if (t.len == 1 && t.end == 0) t.len = 0;
                b.seg.insert(b.seg.begin() + static_cast<std::ptrdiff_t>(from + below(b.seg.size() - from + 1)), t);
                ++hostile_total;
            }
            if (order == 2) std::shuffle(b.seg.begin() + static_cast<std::ptrdiff_t>(from), b.seg.end(), rng);
        }
        b.first.push_back(b.seg.size());
        std::vector<std::vector<Tok>> got;
        if (!run(b, first_ids, cont_ids, unk_id, max_chars, got)) { std::printf("MISMATCH round %d: a lane wrote outside its slice\n", r); return 1; }
        for (uint64_t d = 0; d < n; ++d) {
            std::vector<Tok> want;
            if (b.skip.empty() || !b.skip[d]) want = restate(b.docs[d], order == 3 ? std::vector<Piece>{} : pieces, unk_id, max_chars);
            bool ok = got[d].size() == want.size();
            for (size_t i = 0; ok && i < want.size(); ++i) ok = got[d][i].id == want[i].id && got[d][i].start == want[i].start && got[d][i].end == want[i].end;
            if (!ok) {
                std::printf("MISMATCH round %d document %llu: %zu tokens want %zu\n", r, static_cast<unsigned long long>(d), got[d].size(), want.size());
                return 1;
            }
            toks_total += want.size();
            unk_total += want.size() == 1 && want[0].id == unk_id && want[0].end == b.docs[d].size() && b.docs[d].size() > 1;
        }
        docs_total += n;
    }
    std::printf("OK %d rounds %llu docs %llu tokens %llu unk %llu hostile tuples\n", rounds, static_cast<unsigned long long>(docs_total),
                static_cast<unsigned long long>(toks_total), static_cast<unsigned long long>(unk_total), static_cast<unsigned long long>(hostile_total));
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 3 && std::strcmp(argv[1], "words") == 0) return words_mode(argv[2]);
    if (argc >= 2 && std::strcmp(argv[1], "hostile") == 0)
        return hostile_mode(argc > 2 ? std::atoi(argv[2]) : 2000, argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 20261019ull);
    std::printf("usage: wordpiece_check words <file> | hostile [rounds] [seed]\n");
    return 2;
}
