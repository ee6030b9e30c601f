// Host-only check of tokenize_unigram's per-lane bodies (no GPU needed): unigram_kernels.hip is compiled as plain C++ (DAAC_UNIGRAM_HOST)
// and its forward, count and write bodies are run document by document on random lattices — random text over a small alphabet (with
// UTF-8 continuation bytes), random patterns with "" among them, all occurrences as the tuple list, documents with offsets[0] > 0 and
// empty ones — against a restatement of the definition that shares no code with them.  Ids, spans, tok_offsets and the bits of every
// score must be equal.  Every array has exactly the size the driver gives it, so built with -fsanitize=address,undefined a read or write
// outside a lane's own slice ends the program.
//   usage: unigram_check [lattices] [seed]
// prints "OK <lattices> lattices <docs> docs <tokens> tokens" or "MISMATCH ..." (exit status 1).
#define DAAC_UNIGRAM_HOST
#include "../../daachorse_amd/csrc/unigram_kernels.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace {

struct Tok { uint32_t id; uint64_t start, end; };

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the definition, for one document
float restate(const std::string &doc, const std::vector<daac::UniTuple> &m, const std::vector<float> &scores, float unk, int gap, uint32_t gap_id,
              std::vector<Tok> &out) {
    const size_t L = doc.size();
    std::vector<float> best(L + 1, -INFINITY);
    std::vector<Tok> from(L + 1, Tok{0, 0, 0});
    std::vector<char> has(L + 1, 0);
    best[0] = 0.0f;
    std::vector<size_t> cuts{0};
    for (size_t p = 1; p < L; ++p)
        if (gap == DAAC_GAP_BYTES || (static_cast<uint8_t>(doc[p]) & 0xC0) != 0x80) cuts.push_back(p);
    if (L) cuts.push_back(L);
    for (size_t q = 1; q <= L; ++q) {
        float inc = -INFINITY;
        for (const daac::UniTuple &t : m) {
            if (t.end != q || t.len == 0) continue;
            const size_t s = q - t.len;
            if (best.at(s) == -INFINITY) continue;
            const volatile float c = best[s] + scores.at(t.value);
            if (c > inc) { inc = c; from[q] = Tok{t.value, s, q}; has[q] = 1; }
        }
        for (size_t j = 1; j < cuts.size(); ++j) {
            if (cuts[j] != q || best[cuts[j - 1]] == -INFINITY) continue;
            const volatile float c = best[cuts[j - 1]] + unk;
            if (c > inc) { inc = c; from[q] = Tok{gap_id + (gap == DAAC_GAP_BYTES ? static_cast<uint8_t>(doc[cuts[j - 1]]) : 0u), cuts[j - 1], q}; has[q] = 1; }
        }
        best[q] = inc;
    }
    std::vector<Tok> rev;
    for (size_t q = L; q > 0; q = from[q].start) {
        if (!has[q]) { std::printf("MISMATCH the restatement reached a position without an edge\n"); std::exit(1); }
        rev.push_back(from[q]);
    }
    out.assign(rev.rbegin(), rev.rend());
    return best[L];
}

}  // namespace

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261018ull);
    auto below = [&](uint64_t n) { return static_cast<uint64_t>(rng() % n); };
    const std::string alphabets[3] = {"ab", "abc", std::string("a\x80\xc3\xa9", 4)};
    const float pool[6] = {0.0f, -0.25f, -0.5f, -0.75f, -1.0f, 0.125f};
    uint64_t docs_total = 0, toks_total = 0;
    for (int r = 0; r < rounds; ++r) {
        const std::string &alpha = alphabets[below(3)];
        const int gap = below(2) ? DAAC_GAP_BYTES : DAAC_GAP_CHARS;
        const uint32_t gap_id = below(2) ? 0x10000u : 0xFFFFFF00u;
        const bool ties = below(3) == 0;
        std::vector<std::string> pats;
        if (below(3) == 0) pats.push_back("");
        for (uint64_t i = 0, np = 1 + below(12); i < np; ++i) {
            std::string p;
            for (uint64_t j = 0, l = 1 + below(6); j < l; ++j) p += alpha[below(alpha.size())];
            pats.push_back(p);
        }
        std::vector<float> scores(pats.size() + below(3));
        for (float &s : scores) s = ties ? pool[below(6)] : static_cast<float>(static_cast<int64_t>(below(2000001)) - 1000000) * 1e-5f;
        const float unk = ties ? pool[below(6)] : static_cast<float>(static_cast<int64_t>(below(2000001)) - 1500000) * 1e-5f;
        // the batch: n documents behind `lead` bytes that belong to nobody
        const uint64_t n = 1 + below(6), lead = below(4);
        std::vector<std::string> docs(n);
        std::vector<unsigned long long> off(n + 1, lead), first(n + 1, 0);
        std::vector<uint8_t> text;   // the documents only: a.hay is byte 0 of document 0
        std::vector<daac::UniTuple> seg;
        for (uint64_t d = 0; d < n; ++d) {
            for (uint64_t j = 0, l = below(4) == 0 ? 0 : below(41); j < l; ++j) docs[d] += alpha[below(alpha.size())];
            off[d + 1] = off[d] + docs[d].size();
            text.insert(text.end(), docs[d].begin(), docs[d].end());
            first[d] = seg.size();
            for (uint64_t e = 0; e <= docs[d].size(); ++e)       // every occurrence, by end; at one end in pattern order, longest first now and then
                for (size_t k = 0; k < pats.size(); ++k) {
                    const size_t i = (r & 1) ? pats.size() - 1 - k : k;
                    const std::string &p = pats[i];
                    if (p.size() <= e && docs[d].compare(e - p.size(), p.size(), p) == 0) seg.push_back(daac::UniTuple{e, static_cast<uint32_t>(p.size()), static_cast<uint32_t>(i)});
                }
        }
        first[n] = seg.size();
        const uint64_t len = off[n] - off[0], pos = len + n;
        std::vector<float> best(pos, NAN), doc_scores(n, NAN);
        std::vector<daac::UniBack> back(pos, daac::UniBack{0xFFFFFFFFu, 0xFFFFFFFFu});
        std::vector<unsigned long long> tok_off(n + 1, ~0ull);
        daac::UnigramArgs a{};
        a.hay = text.data();
        a.seg = seg.data();
        a.doc_first = first.data();
        a.doc_off = off.data();
        a.n_docs = n;
        a.scores = scores.data();
        a.n_scores = scores.size();
        a.unk_score = unk;
        a.gap = gap;
        a.gap_id = gap_id;
        a.best = best.data();
        a.back = back.data();
        a.doc_scores = doc_scores.data();
        a.tok_offsets = tok_off.data();
        for (uint64_t d = 0; d < n; ++d) daac::unigram_forward_lane(a, d);
        for (uint64_t d = 0; d < n; ++d) tok_off[d] = daac::unigram_count_lane(a, d);
        unsigned long long run = 0;
        for (uint64_t d = 0; d <= n; ++d) { const unsigned long long c = d < n ? tok_off[d] : 0; tok_off[d] = run; run += c; }
        std::vector<uint32_t> ids(run, 0xDEADBEEFu);
        std::vector<unsigned long long> spans(2 * run, ~0ull);
        a.ids = ids.data();
        a.spans = spans.data();
        for (uint64_t d = 0; d < n; ++d) daac::unigram_write_lane(a, d);
        for (uint64_t d = 0; d < n; ++d) {
            std::vector<Tok> want;
            const std::vector<daac::UniTuple> mine(seg.begin() + first[d], seg.begin() + first[d + 1]);
            const float ws = restate(docs[d], mine, scores, unk, gap, gap_id, want);
            bool ok = bits(ws) == bits(doc_scores[d]) && tok_off[d + 1] - tok_off[d] == want.size();
            for (size_t i = 0; ok && i < want.size(); ++i) {
                const uint64_t x = tok_off[d] + i;
                ok = ids[x] == want[i].id && spans[2 * x] == want[i].start && spans[2 * x + 1] == want[i].end;
            }
            if (!ok) {
                std::printf("MISMATCH lattice %d document %llu: score %08x want %08x, %llu tokens want %zu\n", r, static_cast<unsigned long long>(d), bits(doc_scores[d]),
                            bits(ws), tok_off[d + 1] - tok_off[d], want.size());
                return 1;
            }
            toks_total += want.size();
        }
        docs_total += n;
    }
    std::printf("OK %d lattices %llu docs %llu tokens\n", rounds, static_cast<unsigned long long>(docs_total), static_cast<unsigned long long>(toks_total));
    return 0;
}
