// GRAM engine, `.count()` kernel (gram4_kernels.hip): where a surviving hit's record lies, by a minimal-ish perfect hash (round 10).
//
// A hit that passes the filter of gram4_filter.hpp is, by construction of M, a depth-(K+1) trie state, and all the FILT body wants from it
// is the address of that state's 8-byte record.  Until round 10 it rebuilt the state's RANK for that (context index, four M words, a
// directory entry, four popcounts: 23 VALU and 5 LDS reads a batch); here the address comes from the K+1 RAW bytes the survivor carries:
//
//      h      = g4f_h(x)                         the 24-bit mix the Bloom probe already defines (gram4_filter.hpp)
//      f      = x * a + (x >> 24) * b            a second 24-bit mix, constants from the seed the builder settled on
//      bucket = h * buckets >> 24                one v_mul_hi_u32_u24
//      d      = disp[bucket]                     ONE byte per bucket, in LDS where the coarse rank directory lay
//      slot   = ((f * d + h) mod 2^24) * nh >> shift         v_mad_u32_u24, v_mul_u32_u24, v_lshrrev_b32;  slots = nh << (24 - shift), nh < 256
//
// and the record is dhit_h[slot]: the records of dhit_c permuted into slot order.  Hash and displace: the builder (gram4.cpp) takes the buckets
// by decreasing size and gives each the first d that puts all its keys on free slots.  Only 24-bit multiplies and shifts — the integer ops gfx950
// issues at full rate.  Keys are raw bytes, as the filter's: a dictionary in which a byte class stands for several bytes has neither.
// Shared by the table builder, the kernel and the CPU check (tests/native/gram4_mph_check.cpp).
#pragma once
#include <cstdint>

#include "gram4_filter.hpp"

namespace daac {

struct G4Mph {
    uint32_t bk8;      // buckets << 8 (buckets < 2^16: the bucket is bits 32-47 of a 24 x 24 product)
    uint32_t nh;       // slots = nh << (24 - shift), nh < 256: the slot is a 24 x 8-bit product shifted down
    uint32_t shift;
    uint32_t a, b;     // f's multipliers (odd, 24 bits), from the seed
};

// (device: d comes from LDS, so the multiplier is a vector register here — g4f_mad24 wants it uniform)
DAAC_G4F_HD inline uint32_t g4m_mad24v(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
#else
    return g4f_mul24(a, b) + c;
#endif
}
DAAC_G4F_HD inline uint32_t g4m_f(uint32_t x, const G4Mph &p) { return g4f_mad24(x, p.a, g4f_mul24(x >> 24, p.b)); }
DAAC_G4F_HD inline uint32_t g4m_bucket(uint32_t h, const G4Mph &p) { return g4f_mulhi24(h, p.bk8); }
DAAC_G4F_HD inline uint32_t g4m_slot(uint32_t h, uint32_t f, uint32_t d, const G4Mph &p) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t m;   // (by hand: the compiler does not know that nh has 8 bits and takes the quarter-rate v_mul_lo_u32 for t & 0xffffff)
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(m) : "v"(g4m_mad24v(f, d, h)), "s"(p.nh));
    return m >> p.shift;
#else
    return g4f_mul24(g4m_mad24v(f, d, h), p.nh) >> p.shift;
#endif
}

}  // namespace daac
