// IEEE round-to-nearest-even narrowing of a double to fp16 / bf16 bit patterns in ONE step, written so that the SAME source
// runs inside a HIP kernel (devexport.hip) and in a plain C++ harness (tests/native), where fp16 is held bit for bit to
// numpy's astype and bf16 to an exact-remainder model.  Integer work on the bit pattern only, in the style of fmtdouble.hpp
// and parsedouble.hpp: the g++ build and the gfx950 build give the same bits by construction.
//
// Why one step: a detour over fp32 rounds twice.  65519.999 is 65504 in fp16 but rounds to 65520.0f first, a tie that then
// goes to inf; 1 + 2^-11 + 2^-40 is above the fp16 tie, but its fp32 value is the tie itself and goes down to 1.
//
// x = (-1)^s m 2^(E - 52), m the 53-bit significand.  The target keeps MB fraction bits: a normal result drops
// 52 - MB bits of m, a result below the target's smallest normal drops 1 - (E + bias) more (the subnormal grid
// 2^(1 - bias - MB)); the dropped bits decide by their exact value against half a unit, a tie goes to the even quotient.
// The quotient is ADDED to the exponent field, so a significand that rounds up to 2^(MB + 1) carries into the exponent,
// a subnormal that rounds up to 2^MB becomes the smallest normal, and the largest finite value's upper half becomes inf.
// fp64 subnormals and everything else below a quarter of the target's smallest subnormal are +-0; NaN stays a quiet NaN
// with its sign and the top MB - 1 payload bits.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef GD_HD
#ifdef __HIPCC__
#define GD_HD __host__ __device__
#else
#define GD_HD
#endif
#endif

namespace gdcvt {

GD_HD inline uint64_t f64_bits(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(x);
#else
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
#endif
}

// the pattern of a binary float with EB exponent bits and MB fraction bits (EB + MB + 1 <= 16 here)
template <int EB, int MB>
GD_HD inline uint32_t narrow_bits(uint64_t b) {
    const uint32_t sign = (uint32_t)(b >> 63) << (EB + MB);
    const uint32_t exp_all = ((1u << EB) - 1u) << MB;
    const int e = (int)((b >> 52) & 0x7ffu);
    const uint64_t frac = b & 0xfffffffffffffULL;
    if (e == 0x7ff) {
        if (frac == 0) return sign | exp_all;
        return sign | exp_all | (1u << (MB - 1)) | (uint32_t)(frac >> (52 - MB));
    }
    if (e == 0) return sign;  // zero, and fp64 subnormals: far below half the smallest subnormal of either target
    const int bias = (1 << (EB - 1)) - 1;
    int te = e - 1023 + bias;  // the biased exponent of a normal result
    if (te >= (1 << EB) - 1) return sign | exp_all;
    int shift = 52 - MB;
    if (te <= 0) shift += 1 - te, te = 0;
    if (shift >= 54) return sign;  // m < 2^53: below half a unit of the subnormal grid
    const uint64_t m = frac | (1ULL << 52);
    uint64_t q = m >> shift;
    const uint64_t rem = m & ((1ULL << shift) - 1ULL), half = 1ULL << (shift - 1);
    if (rem > half || (rem == half && (q & 1ULL))) ++q;
    // a normal q holds the implicit one (2^MB): it counts as one step of the exponent field
    const uint32_t bits = ((uint32_t)(te > 0 ? te - 1 : 0) << MB) + (uint32_t)q;
    return sign | (bits >= exp_all ? exp_all : bits);
}

GD_HD inline uint16_t f64_to_f16_bits(double x) { return (uint16_t)narrow_bits<5, 10>(f64_bits(x)); }
GD_HD inline uint16_t f64_to_bf16_bits(double x) { return (uint16_t)narrow_bits<8, 7>(f64_bits(x)); }
// fp32: the plain cast is a single rounding in hardware (v_cvt_f32_f64; subnormal results are kept, the kernels run with
// fp32 denormals on)
GD_HD inline float f64_to_f32(double x) { return (float)x; }

}  // namespace gdcvt
