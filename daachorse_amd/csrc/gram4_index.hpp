// GRAM engine, `.count()` kernel (gram4_kernels.hip): the LDS address of a position's M word, K = 3, shared between the two positions of
// a pair (round 11).
//
// The M word of the 3-gram ending at position j lies at  A_j = offM + 4 c_j + 4 C c_(j-1) + 4 C^2 c_(j-2)  (c = byte class, C classes).  Worked
// out on its own that is a v_lshl_add_u32 and two v_mad_u32_u24 a position.  The intermediate of an even position,
//     q_j = offM + 4 c_j + 4 C c_(j-1),
// holds everything the next position needs of c_j and c_(j-1):
//     A_(j+1) = C q_j + (4 c_(j+1) + offM - C offM)
// — one v_lshl_add_u32 with a second constant (offM1 = offM - C offM, wrapping in 32 bits as the multiply-add's sum does) and ONE
// v_mad_u32_u24: five instructions a pair instead of six.  q_j is an LDS address (below 160 KB), so it fits the 24-bit multiplier.
// Shared by the kernel and the CPU check (tests/native/gram4_index_check.cpp walks every class tuple through both forms).
#pragma once
#include <cstdint>

#include "gram4_filter.hpp"

namespace daac {

struct G4Idx { uint32_t addr, q; };   // LDS address of the M word; the intermediate the next position multiplies

// (c << 2) + k as one v_lshl_add_u32 (device: pinned — left to itself the compiler folds the constant into the multiply-adds' operands)
DAAC_G4F_HD inline uint32_t g4i_lshl2_add(uint32_t c, uint32_t k) {
    uint32_t x = (c << 2) + k;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}
// the second constant of an odd position: offM - C offM (mod 2^32)
DAAC_G4F_HD inline uint32_t g4i_off1(uint32_t offM, uint32_t C) { return offM - C * offM; }
// even position j: c_j, c_j1 = c_(j-1), c_j2 = c_(j-2)
DAAC_G4F_HD inline G4Idx g4i_even(uint32_t c_j, uint32_t c_j1, uint32_t c_j2, uint32_t offM, uint32_t C) {
    G4Idx r;
    r.q = g4f_mad24(c_j1, C * 4u, g4i_lshl2_add(c_j, offM));
    r.addr = g4f_mad24(c_j2, C * C * 4u, r.q);
    return r;
}
// odd position j: q of position j - 1, c_j, offM1 = g4i_off1(offM, C)
DAAC_G4F_HD inline uint32_t g4i_odd(uint32_t q, uint32_t c_j, uint32_t offM1, uint32_t C) {
    return g4f_mad24(q, C, g4i_lshl2_add(c_j, offM1));
}

}  // namespace daac
