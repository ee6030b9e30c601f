// Host-only check of tokenize_bpe's per-lane bodies (no GPU needed): bpe_kernels.hip is compiled as plain C++ (DAAC_BPE_HOST) and its
// merge and write bodies are run document by document on random inputs — random text over a small alphabet (with UTF-8 continuation
// bytes), random patterns with "" among them, all occurrences as the tuple list (tuples that share an end in either order), rank tables
// with equal ranks and 0xFFFFFFFF in them, documents with offsets[0] > 0, empty ones and one beyond doc_max — against a restatement of
// the definition that shares no code with them.  Ids, spans and tok_offsets must be equal.  Every array has exactly the size the driver
// gives it, so built with -fsanitize=address,undefined a read or write outside a lane's own slice ends the program.
//   usage: bpe_check [rounds] [seed]
// prints "OK <rounds> rounds <docs> docs <tokens> tokens" or "MISMATCH ..." (exit status 1).
#define DAAC_BPE_HOST
#include "../../daachorse_amd/csrc/bpe_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

namespace {

struct Tok { uint32_t id; uint64_t start, end; };

// the definition, for one document
void restate(const std::string &doc, const std::vector<daac::BpeTuple> &m, const std::vector<uint32_t> *ranks, int gap, uint32_t gap_id, std::vector<Tok> &out) {
    const size_t L = doc.size();
    out.clear();
    if (!L) return;
    std::map<std::pair<size_t, size_t>, uint32_t> piece;
    for (const daac::BpeTuple &t : m)
        if (t.len) piece[{t.end - t.len, t.end}] = t.value;
    std::vector<size_t> b{0};
    for (size_t p = 1; p < L; ++p)
        if (gap == DAAC_GAP_BYTES || (static_cast<uint8_t>(doc[p]) & 0xC0) != 0x80) b.push_back(p);
    b.push_back(L);
    for (;;) {
        uint64_t best = 0xFFFFFFFFull;
        size_t at = 0;
        for (size_t i = 0; i + 2 < b.size(); ++i) {
            const auto it = piece.find({b[i], b[i + 2]});
            if (it == piece.end()) continue;
            const uint64_t r = ranks ? ranks->at(it->second) : it->second;
            if (r < best) { best = r; at = i; }
        }
        if (best == 0xFFFFFFFFull) break;
        b.erase(b.begin() + static_cast<std::ptrdiff_t>(at) + 1);
    }
    for (size_t i = 0; i + 1 < b.size(); ++i) {
        const auto it = piece.find({b[i], b[i + 1]});
        const uint32_t id = it != piece.end() ? it->second : gap_id + (gap == DAAC_GAP_BYTES ? static_cast<uint8_t>(doc[b[i]]) : 0u);
        out.push_back(Tok{id, b[i], b[i + 1]});
    }
}

}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261018ull);
    auto below = [&](uint64_t n) { return static_cast<uint64_t>(rng() % n); };
    const std::string alphabets[3] = {"ab", "abc", std::string("a\x80\xc3\xa9", 4)};
    uint64_t docs_total = 0, toks_total = 0;
    for (int r = 0; r < rounds; ++r) {
        const std::string &alpha = alphabets[below(3)];
        const int gap = below(2) ? DAAC_GAP_BYTES : DAAC_GAP_CHARS;
        const uint32_t gap_id = below(2) ? 0x10000u : 0xFFFFFF00u;
        std::vector<std::string> pats;
        if (below(3) == 0) pats.push_back("");
        for (uint64_t i = 0, np = 1 + below(14); i < np; ++i) {
            std::string p;
            for (uint64_t j = 0, l = 1 + below(below(4) ? 3 : 6); j < l; ++j) p += alpha[below(alpha.size())];
            bool seen = false;
            for (const std::string &q : pats) seen = seen || q == p;
            if (!seen) pats.push_back(p);   // patterns are unique
        }
        // values: the index, or scattered; ranks: none, or a table with few distinct ranks and 0xFFFFFFFF now and then
        std::vector<uint32_t> values(pats.size());
        const bool scattered = below(3) == 0;
        for (size_t i = 0; i < pats.size(); ++i) values[i] = scattered ? static_cast<uint32_t>(3 * (pats.size() - 1 - i) + 1) : static_cast<uint32_t>(i);
        const uint64_t kind = below(3);   // 0: no table
        std::vector<uint32_t> ranks;
        if (kind) {
            ranks.resize(3 * pats.size() + 2 + below(3));
            for (uint32_t &x : ranks) x = below(8) == 0 ? 0xFFFFFFFFu : kind == 1 ? static_cast<uint32_t>(below(3)) : static_cast<uint32_t>(below(1000));
        }
        // the batch: n documents behind `lead` bytes that belong to nobody
        const uint64_t n = 1 + below(6), lead = below(4), doc_max = 40;
        std::vector<std::string> docs(n);
        std::vector<unsigned long long> off(n + 1, lead), first(n + 1, 0);
        std::vector<uint8_t> text;   // the documents only: a.hay is byte 0 of document 0
        std::vector<daac::BpeTuple> seg;
        for (uint64_t d = 0; d < n; ++d) {
            for (uint64_t j = 0, l = below(4) == 0 ? 0 : below(20) == 0 ? 41 + below(3) : below(41); j < l; ++j) docs[d] += alpha[below(alpha.size())];
            off[d + 1] = off[d] + docs[d].size();
            text.insert(text.end(), docs[d].begin(), docs[d].end());
            first[d] = seg.size();
            for (uint64_t e = 0; e <= docs[d].size(); ++e)       // every occurrence, by end; at one end in pattern order, or the other way round
                for (size_t k = 0; k < pats.size(); ++k) {
                    const size_t i = (r & 1) ? pats.size() - 1 - k : k;
                    const std::string &p = pats[i];
                    if (p.size() <= e && docs[d].compare(e - p.size(), p.size(), p) == 0) seg.push_back(daac::BpeTuple{e, static_cast<uint32_t>(p.size()), values[i]});
                }
        }
        first[n] = seg.size();
        const uint64_t len = off[n] - off[0], pos = len + n;
        std::vector<daac::BpeSlot> slots(pos, daac::BpeSlot{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu});
        std::vector<unsigned long long> tok_off(n + 1, ~0ull);
        daac::BpeArgs a{};
        a.hay = text.data();
        a.seg = seg.data();
        a.doc_first = first.data();
        a.doc_off = off.data();
        a.n_docs = n;
        a.ranks = kind ? ranks.data() : nullptr;
        a.n_ranks = ranks.size();
        a.doc_max = doc_max;
        a.gap = gap;
        a.gap_id = gap_id;
        a.slots = slots.data();
        a.tok_offsets = tok_off.data();
        for (uint64_t d = 0; d < n; ++d) tok_off[d] = daac::bpe_merge_lane(a, d);
        unsigned long long run = 0;
        for (uint64_t d = 0; d <= n; ++d) { const unsigned long long c = d < n ? tok_off[d] : 0; tok_off[d] = run; run += c; }
        std::vector<uint32_t> ids(run, 0xDEADBEEFu);
        std::vector<unsigned long long> spans(2 * run, ~0ull);
        a.ids = ids.data();
        a.spans = spans.data();
        for (uint64_t d = 0; d < n; ++d) daac::bpe_write_lane(a, d);
        for (uint64_t d = 0; d < n; ++d) {
            std::vector<Tok> want;
            const std::vector<daac::BpeTuple> mine(seg.begin() + static_cast<std::ptrdiff_t>(first[d]), seg.begin() + static_cast<std::ptrdiff_t>(first[d + 1]));
            if (docs[d].size() <= doc_max) restate(docs[d], mine, kind ? &ranks : nullptr, gap, gap_id, want);   // beyond doc_max: left alone, no tokens
            bool ok = tok_off[d + 1] - tok_off[d] == want.size();
            for (size_t i = 0; ok && i < want.size(); ++i) {
                const uint64_t x = tok_off[d] + i;
                ok = ids[x] == want[i].id && spans[2 * x] == want[i].start && spans[2 * x + 1] == want[i].end;
            }
            if (!ok) {
                std::printf("MISMATCH round %d document %llu: %llu tokens want %zu\n", r, static_cast<unsigned long long>(d), tok_off[d + 1] - tok_off[d], want.size());
                return 1;
            }
            toks_total += want.size();
        }
        docs_total += n;
    }
    std::printf("OK %d rounds %llu docs %llu tokens\n", rounds, static_cast<unsigned long long>(docs_total), static_cast<unsigned long long>(toks_total));
    return 0;
}
