// numpy's default bit generator, PCG64 (128-bit LCG state, XSL-RR 128/64 output), written so that the SAME source runs
// inside a HIP kernel and in a plain C++ harness (tests/native), where it is checked bit for bit against
// np.random.default_rng(seed).random(n).
//
// The state steps  s <- s * MULT + inc  (mod 2^128); an LCG composes: k steps are again an affine map
// s -> a_k s + c_k, and (a_k, c_k) follow from the binary digits of k in O(log k) 128-bit multiplies (F. Brown, "Random
// number generation with arbitrary strides", 1994 -- the jump-ahead numpy's PCG64.advance uses).  So every thread of a
// kernel can start at its own row (advance) and then walk rows t, t + T, t + 2T, ... with one multiply-add per row
// (stride(T)).  Generator.random() of numpy takes the top 53 bits of one 64-bit output: draw i (0-based) of a generator
// whose bit_generator.state holds (state, inc) is  next_double  after  advance(i): the step comes first, the output is of
// the NEW state.  A pending 32-bit half (has_uint32) plays no part in the doubles.
//
// No tables, no global state.
#pragma once
#include <stdint.h>

#ifndef GD_HD
#ifdef __HIPCC__
#define GD_HD __host__ __device__
#else
#define GD_HD
#endif
#endif

namespace gdpcg {

typedef unsigned __int128 u128;

GD_HD inline u128 make_u128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | (u128)lo; }
GD_HD inline uint64_t hi64(u128 v) { return (uint64_t)(v >> 64); }
GD_HD inline uint64_t lo64(u128 v) { return (uint64_t)v; }

// PCG_DEFAULT_MULTIPLIER_128
GD_HD inline u128 multiplier() { return make_u128(0x2360ED051FC65DA4ULL, 0x4385DF649FCCF645ULL); }

// the affine map s -> a s + c (mod 2^128)
struct Affine {
    u128 a, c;
    GD_HD u128 operator()(u128 s) const { return a * s + c; }
};

// k steps of the generator with increment `inc` as one map: (MULT^k, inc (MULT^k - 1) / (MULT - 1))
GD_HD inline Affine stride(u128 inc, u128 k) {
    Affine acc = {(u128)1, (u128)0};
    u128 cur_a = multiplier(), cur_c = inc;
    while (k > 0) {
        if (k & 1) {
            acc.a *= cur_a;
            acc.c = acc.c * cur_a + cur_c;
        }
        cur_c = (cur_a + 1) * cur_c;
        cur_a *= cur_a;
        k >>= 1;
    }
    return acc;
}

// XSL-RR: xor the halves, rotate right by the top six bits of the state
GD_HD inline uint64_t output(u128 s) {
    const uint64_t x = hi64(s) ^ lo64(s);
    const unsigned rot = (unsigned)(s >> 122);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

// 53 random bits as a double in [0, 1): what Generator.random() makes of one 64-bit output
GD_HD inline double to_double(uint64_t x) { return (double)(x >> 11) * (1.0 / 9007199254740992.0); }

struct Pcg64 {
    u128 state, inc;

    GD_HD void advance(u128 delta) { state = stride(inc, delta)(state); }
    GD_HD uint64_t next_u64() {
        state = state * multiplier() + inc;
        return output(state);
    }
    GD_HD double next_double() { return to_double(next_u64()); }
};

}  // namespace gdpcg
