// CPU check of gram4_index.hpp (the pair-shared M-word address of gram4_kernels.hip's main path, K = 3): for every class count C in 2..30,
// four places of M in LDS (0, 16, the middle, the highest 16-byte aligned one at which M still ends inside 160 KB) and every class tuple
// (c0, c1, c2, c3) below C, the odd position's address from the even position's intermediate equals the three-term address of (c1, c2, c3),
// the even position's own address equals that of (c0, c1, c2), and every operand of a 24-bit multiply-add is below 2^24 (the host form of
// g4f_mad24 masks its factors to 24 bits as the instruction does, so a wider one would also show as a wrong address).
// Prints "OK tuples=<n>" or the first failure.
#include <cstdint>
#include <cstdio>

#include "../../daachorse_amd/csrc/gram4_index.hpp"

using namespace daac;

static uint32_t old_addr(uint32_t c_j, uint32_t c_j1, uint32_t c_j2, uint32_t offM, uint32_t C) {
    return offM + 4u * c_j + 4u * C * c_j1 + 4u * C * C * c_j2;
}

int main() {
    constexpr uint32_t kLds = 163840u, kLim = 1u << 24;
    unsigned long long tuples = 0;
    for (uint32_t C = 2; C <= 30; ++C) {
        const uint32_t m_bytes = 4u * C * C * C;
        const uint32_t offs[4] = {0u, 16u, 81920u, (kLds - 4u - m_bytes) & ~15u};
        for (uint32_t offM : offs) {
            const uint32_t offM1 = g4i_off1(offM, C);
            if (C >= kLim || 4u * C >= kLim || 4u * C * C >= kLim) { std::printf("FAIL uniform operand C=%u\n", C); return 1; }
            for (uint32_t c0 = 0; c0 < C; ++c0)
                for (uint32_t c1 = 0; c1 < C; ++c1)
                    for (uint32_t c2 = 0; c2 < C; ++c2) {
                        const G4Idx e = g4i_even(c2, c1, c0, offM, C);
                        if (e.addr != old_addr(c2, c1, c0, offM, C)) {
                            std::printf("FAIL even C=%u offM=%u c=(%u,%u,%u) addr=%u\n", C, offM, c0, c1, c2, e.addr);
                            return 1;
                        }
                        if (e.q >= kLim || c0 >= kLim || c1 >= kLim) {
                            std::printf("FAIL operand C=%u offM=%u c=(%u,%u,%u) q=%u\n", C, offM, c0, c1, c2, e.q);
                            return 1;
                        }
                        for (uint32_t c3 = 0; c3 < C; ++c3) {
                            const uint32_t got = g4i_odd(e.q, c3, offM1, C), want = old_addr(c3, c2, c1, offM, C);
                            if (got != want) {
                                std::printf("FAIL odd C=%u offM=%u c=(%u,%u,%u,%u) got=%u want=%u\n", C, offM, c0, c1, c2, c3, got, want);
                                return 1;
                            }
                            ++tuples;
                        }
                    }
        }
    }
    std::printf("OK tuples=%llu\n", tuples);
    return 0;
}
