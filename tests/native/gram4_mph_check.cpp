// Host-logic test for the perfect hash over the depth-(K+1) states (gram4_mph.hpp, build_gram4_mph; no GPU needed): every key — a
// (K+1)-gram with a continuation bit in M, named by its raw bytes — maps to a slot of its own below mph_slots, the record in that slot is the
// one the key's RANK names (the rank worked out as gram4_kernels.hip's rank_and_ask does: coarse directory + the words of the group before
// the hit's + the bits below the hit's), unused slots are zero, the displacement table is no larger than the coarse directory it replaces
// in LDS, dhit_h at most twice dhit_c, and a second build gives the same bytes.  Then the text is walked as the FILT body walks it — probe of
// gram4_filter.hpp, survivors' records by hash and by rank — and the pattern ends and go-ons counted both ways must be equal.
//   usage: gram4_mph_check <blob> <lds_budget> <haystack-file> [seeds] [filter-bytes]
// prints OK ..., DECLINED ... (the builder said no: the handle keeps the rank path) or MISMATCH ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../daachorse_amd/csrc/gram4.hpp"
#include "../../daachorse_amd/csrc/pma.hpp"

using namespace daac;

static std::vector<uint8_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::vector<uint8_t> blob = slurp(argv[1]);
    HostPma p;
    if (HostPma::deserialize(blob.data(), blob.size(), p, nullptr) != DAAC_OK) { std::printf("BADBLOB\n"); return 1; }
    Gram2Tables g2;
    if (!build_gram2_tables(p, static_cast<uint32_t>(std::atoi(argv[2])), g2)) { std::printf("UNAVAILABLE gram2\n"); return 0; }
    Gram4Tables g;
    build_gram4_tables(g2, g);
    if (!g.available) { std::printf("MISMATCH gram4 not built\n"); return 1; }
    const uint32_t seeds = argc > 4 ? static_cast<uint32_t>(std::atoi(argv[4])) : kGram4MphSeeds;
    const uint32_t fbytes = argc > 5 ? static_cast<uint32_t>(std::atoi(argv[5])) : 33000u;
    const uint32_t K = g.K, C = g.C, OTH = C - 1;
    // bytes of the coarse directory as the kernel stages it (u16 entries beside a per-word directory, else u32; 16-byte pieces)
    const uint32_t s_bytes = static_cast<uint32_t>((g.sdir.size() * (g.s16 ? 2 : 4) + 15) & ~size_t{15});
    const size_t n = g.dhit_c.size();
    if (!build_gram4_mph(g, s_bytes, seeds)) {
        if (!g.mph_disp.empty() || !g.dhit_h.empty() || g.mph_slots != 0) { std::printf("MISMATCH declined but left tables\n"); return 1; }
        std::printf("DECLINED K=%u C=%u keys=%zu s_bytes=%u seeds=%u s16=%d n_deep=%zu\n", K, C, n, s_bytes, seeds, g.s16 ? 1 : 0, n);
        return 0;
    }
    if (g.mph_disp.size() > s_bytes || g.mph_disp.size() % 16 != 0 || g.mph_disp.size() != (g.mph.bk8 >> 8)) { std::printf("MISMATCH displacement table %zu bytes, directory %u\n", g.mph_disp.size(), s_bytes); return 1; }
    if (g.dhit_h.size() != g.mph_slots || g.mph_slots > 2 * n || g.mph_slots < n || g.mph_slots != (g.mph.nh << (24 - g.mph.shift)) || g.mph.nh >= 256) { std::printf("MISMATCH slots %u keys %zu\n", g.mph_slots, n); return 1; }
    if (g.mph_seed == 0 || g.mph_seed > seeds) { std::printf("MISMATCH seed\n"); return 1; }
    {   // two builds, the same bytes
        Gram4Tables h = g;
        if (!build_gram4_mph(h, s_bytes, seeds) || h.mph_disp != g.mph_disp || h.mph_seed != g.mph_seed || h.mph_slots != g.mph_slots ||
            std::memcmp(&h.mph, &g.mph, sizeof(G4Mph)) != 0 || std::memcmp(h.dhit_h.data(), g.dhit_h.data(), g.dhit_h.size() * sizeof(U32x2)) != 0) {
            std::printf("MISMATCH second build differs\n");
            return 1;
        }
    }
    uint32_t byte_of[32] = {0};
    for (uint32_t b = 0; b < 256; ++b) if (g.cls[b] < OTH) byte_of[g.cls[b]] = b;
    auto slot_of = [&](uint32_t x) -> uint32_t {
        const uint32_t h = g4f_h(x), b = g4m_bucket(h, g.mph);
        if (b >= g.mph_disp.size()) return 0xffffffffu;
        return g4m_slot(h, g4m_f(x, g.mph), g.mph_disp[b], g.mph);
    };
    auto rank_of = [&](uint32_t ctx, uint32_t d) -> uint32_t {   // rank_and_ask, coarse directory
        uint32_t rank = g.sdir[ctx >> 2] + static_cast<uint32_t>(__builtin_popcount(g.m[ctx] & ((1u << d) - 1u)));
        for (uint32_t i = ctx & ~3u; i < ctx; ++i) rank += static_cast<uint32_t>(__builtin_popcount(g.m[i] & kGram4ChildBits));
        return rank;
    };
    // every key
    uint64_t ngram = 1;
    for (uint32_t i = 0; i < K; ++i) ngram *= C;
    std::vector<uint8_t> used(g.mph_slots, 0);
    size_t keys = 0;
    for (uint64_t ctx = 0; ctx < ngram; ++ctx) {
        uint32_t xc = 0;
        uint64_t rest = ctx;
        for (uint32_t i = 0; i < K; ++i) { xc |= byte_of[rest % C] << (8 * (K - 1 - i)); rest /= C; }
        for (uint32_t w = g.m[ctx] & kGram4ChildBits; w != 0; w &= w - 1, ++keys) {
            const uint32_t d = static_cast<uint32_t>(__builtin_ctz(w));
            const uint32_t x = xc | (byte_of[d] << (8 * K));
            const uint32_t s = slot_of(x), rank = rank_of(static_cast<uint32_t>(ctx), d);
            if (s >= g.mph_slots) { std::printf("MISMATCH slot out of range (key %08x)\n", x); return 1; }
            if (used[s]) { std::printf("MISMATCH two keys on slot %u\n", s); return 1; }
            used[s] = 1;
            if (rank >= n || g.dhit_h[s].x != g.dhit_c[rank].x || g.dhit_h[s].y != g.dhit_c[rank].y) { std::printf("MISMATCH record of key %08x\n", x); return 1; }
        }
    }
    if (keys != n) { std::printf("MISMATCH %zu keys, %zu records\n", keys, n); return 1; }
    for (uint32_t s = 0; s < g.mph_slots; ++s)
        if (!used[s] && (g.dhit_h[s].x | g.dhit_h[s].y) != 0) { std::printf("MISMATCH unused slot %u not zero\n", s); return 1; }

    // the text, as the FILT body walks it: hit -> probe -> survivors' records, by rank and by hash
    const std::vector<uint8_t> hay = slurp(argv[3]);
    const long long len = static_cast<long long>(hay.size());
    const bool have_filter = build_gram4_filter(g, fbytes);
    const uint32_t W = static_cast<uint32_t>(g.bloom.size());
    auto cls = [&](long long pos) -> uint32_t { return (pos >= 0 && pos < len) ? g.cls[hay[pos]] : OTH; };
    auto raw = [&](long long pos) -> uint32_t { return (pos >= 0 && pos < len) ? hay[pos] : g.unused_byte; };
    uint64_t hits = 0, passed = 0, ends_r = 0, ends_h = 0, go_r = 0, go_h = 0;
    for (long long pz = 0; pz < len; ++pz) {
        uint32_t ctx = 0;
        for (uint32_t t = 0; t < K; ++t) ctx = ctx * C + cls(pz - K + t);
        const uint32_t d = cls(pz);
        if (!((g.m[ctx] >> d) & 1u) || d == OTH) continue;
        ++hits;
        uint32_t x = 0;
        for (uint32_t i = 0; i <= K; ++i) x |= raw(pz - K + i) << (8 * i);
        if (have_filter) {
            const G4Probe pr = g4f_probe(x, raw(pz + 1), W);
            const uint32_t fw = g.bloom[pr.word];
            if (!((fw & pr.go) == pr.go || (fw & pr.ends) == pr.ends)) continue;
        }
        ++passed;
        const uint32_t s = slot_of(x);
        if (s >= g.mph_slots) { std::printf("MISMATCH slot out of range at position %lld\n", pz); return 1; }
        const U32x2 rr = g.dhit_c[rank_of(ctx, d)], rh = g.dhit_h[s];
        const uint32_t k1 = cls(pz + 1);
        ends_r += (rr.x >> kGram4EndsBit) & 1u;
        ends_h += (rh.x >> kGram4EndsBit) & 1u;
        go_r += (rr.x >> k1) & 1u & (k1 < OTH ? 1u : 0u);
        go_h += (rh.x >> k1) & 1u & (k1 < OTH ? 1u : 0u);
        if (rr.x != rh.x || rr.y != rh.y) { std::printf("MISMATCH record at position %lld\n", pz); return 1; }
    }
    if (ends_r != ends_h || go_r != go_h) { std::printf("MISMATCH ends %llu / %llu go-ons %llu / %llu\n", (unsigned long long)ends_r, (unsigned long long)ends_h, (unsigned long long)go_r, (unsigned long long)go_h); return 1; }
    std::printf("OK K=%u C=%u keys=%zu buckets=%zu s_bytes=%u slots=%u seed=%u filter=%d hits=%llu passed=%llu ends=%llu goons=%llu s16=%d n_deep=%zu\n", K, C, n, g.mph_disp.size(), s_bytes,
                g.mph_slots, g.mph_seed, have_filter ? 1 : 0, (unsigned long long)hits, (unsigned long long)passed, (unsigned long long)ends_h, (unsigned long long)go_h, g.s16 ? 1 : 0, n);
    return 0;
}
