// Host-side helper of tests/test_gpu_gram4_survivors.py (no GPU needed): walks a text as gram4's FILT body walks it and writes, for every hit
// in text order — a (K+1)-gram ending at byte p that is a trie prefix —, one u32: p | passed << 31, where `passed` is the probe of
// gram4_filter.hpp against the Bloom array.  The tables are built as the upload builds them (upload_layout.hpp, gram2 and gram4: the table budget less the hit
// rings, the perfect hash first when asked for, the Bloom array in the room gram4_filter_room leaves less 512 bytes), so the array is the
// one the kernel stages.
//   usage: gram4_survivors_check <blob> <haystack-file> <mph: 0 | 1> <out-file>
// prints OK K= C= words= keys= hits= passed=, or NOFILTER / UNAVAILABLE
#include <cstdio>
#include <cstdlib>
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
    if (argc < 5) return 2;
    const std::vector<uint8_t> blob = slurp(argv[1]);
    HostPma p;
    if (HostPma::deserialize(blob.data(), blob.size(), p, nullptr) != DAAC_OK) { std::printf("BADBLOB\n"); return 1; }
    Gram2Tables g2;
    if (!build_gram2_tables(p, 158u * 1024u - 16u * 128u * 8u, g2)) { std::printf("UNAVAILABLE gram2\n"); return 0; }
    Gram4Tables g;
    build_gram4_tables(g2, g);
    if (!g.available) { std::printf("UNAVAILABLE gram4\n"); return 0; }
    auto p16 = [](size_t x) { return static_cast<uint32_t>((x + 15) & ~size_t{15}); };
    const uint32_t m_bytes = p16(g.m.size() * 4), s_bytes = p16(g.sdir.size() * (g.s16 ? 2 : 4));
    uint32_t front = s_bytes;
    if (std::atoi(argv[3]) != 0 && build_gram4_mph(g, s_bytes, kGram4MphSeeds)) front = static_cast<uint32_t>(g.mph_disp.size());
    // gram4_filter_room: sixteen hit lists of 256 u16 entries, sixteen text slots of 32 positions per lane, the class table, the front table, M
    const uint32_t fixed = 16u * 256u * 2u + 16u * (64u * 32u + 32u) + (g.arith ? 0u : 256u) + front + m_bytes, limit = 160u * 1024u;
    const uint32_t room = fixed < limit ? (limit - fixed) & ~15u : 0u;
    if (room <= 1024u || !build_gram4_filter(g, room - 512u)) { std::printf("NOFILTER room=%u\n", room); return 0; }
    const uint32_t K = g.K, C = g.C, OTH = C - 1, W = static_cast<uint32_t>(g.bloom.size());
    const std::vector<uint8_t> hay = slurp(argv[2]);
    const long long len = static_cast<long long>(hay.size());
    auto cls = [&](long long pos) -> uint32_t { return (pos >= 0 && pos < len) ? g.cls[hay[pos]] : OTH; };
    auto raw = [&](long long pos) -> uint32_t { return (pos >= 0 && pos < len) ? hay[pos] : g.unused_byte; };
    std::vector<uint32_t> out;
    uint64_t passed = 0;
    for (long long pz = 0; pz < len; ++pz) {
        uint32_t ctx = 0;
        for (uint32_t t = 0; t < K; ++t) ctx = ctx * C + cls(pz - K + t);
        const uint32_t d = cls(pz);
        if (d == OTH || !((g.m[ctx] >> d) & 1u)) continue;
        uint32_t x = 0;
        for (uint32_t i = 0; i <= K; ++i) x |= raw(pz - K + i) << (8 * i);
        const G4Probe pr = g4f_probe(x, raw(pz + 1), W);
        const uint32_t fw = g.bloom[pr.word];
        const bool pass = (fw & pr.go) == pr.go || (fw & pr.ends) == pr.ends;
        passed += pass;
        out.push_back(static_cast<uint32_t>(pz) | (pass ? 1u << 31 : 0u));
    }
    std::ofstream f(argv[4], std::ios::binary);
    f.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(out.size() * sizeof(uint32_t)));
    if (!f) { std::printf("WRITEFAILED\n"); return 1; }
    std::printf("OK K=%u C=%u words=%u keys=%u hits=%zu passed=%llu\n", K, C, W, g.filter_keys, out.size(), (unsigned long long)passed);
    return 0;
}
