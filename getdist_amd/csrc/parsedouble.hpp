// Decimal token -> IEEE double, the inverse of fmtdouble.hpp, written so that the SAME source runs inside a HIP kernel
// (ingest.hip) and in a plain C++ harness (tests/native), where it is held bit for bit to np.loadtxt.  Integer arithmetic
// only -- no floating-point operation, no libm -- so the g++ build and the gfx950 build give the same bits by construction.
//
// Grammar (what np.loadtxt takes for a float field): [+-] digits with at most one '.' and at least one digit, an optional
// exponent [eE][+-]digits; or [+-] nan | inf | infinity in any letter case.  Everything else -- '_', hex, a Fortran 'd'
// exponent, 'j', a bare 'e', any byte >= 0x80 or NUL, the empty token -- is GD_PARSE_NAN_TOKEN ("not a number").
//
// Value: the first 19 significant digits make w < 10^19 < 2^64 and the token is  w 10^q  (plus a tail below one unit of w
// when more digits follow).  With w64 = w << lz (bit 63 set) and T = POW10_128[q] = floor(10^q 2^-e), e = floor(q log2 10)
// - 127 (scripts/gen_fmtdouble_table.py: 10^q = (T + d) 2^e, 0 <= d < 1, d = 0 exactly for 0 <= q <= 55), the 192-bit
// product P = w64 T satisfies
//     w 10^q = (P + w64 d) 2^(e - lz),      0 <= w64 d < 2^64,
// so the true product lies in [P, P + 2^64), and in {P} when the entry is exact.  P has its top bit at n = 190 or 191.
// A double keeps k = 53 bits of it (0 .. 52 for a subnormal result), i.e. drops the low s = n + 1 - k >= 138 bits: with
// R = P mod 2^s and H = 2^(s-1) the result is floor(P / 2^s), plus one when the true remainder is above H, or equal to H
// with an odd quotient.
//   exact entry:   the remainder is R itself: all three cases are decided, ties included;
//   inexact entry: the true remainder is R + t with 0 < t < 2^64 (d > 0: 10^q has no 128-bit binary form outside 0..55).
//                  R >= H: above H, round up (a carry past 2^s gives the same double: quotient + 1 with a small remainder).
//                  R < H - 2^64: below H, round down.  Otherwise -- R within 2^64 below H, a window of relative width
//                  2^64 / 2^(s-1) <= 2^-73 of a unit in the last place -- the token is GD_PARSE_UNDECIDED.
//   In units of 2^64 (hi = P >> 64, Rhi = R >> 64, Hhi = H >> 64; s >= 138, so H is a multiple of 2^64):
//                  up when Rhi >= Hhi, undecided when Rhi == Hhi - 1, down when Rhi < Hhi - 1.
// More than 19 significant digits: when the dropped digits are all zero the token equals w 10^q.  Otherwise it lies
// strictly between w 10^q and (w + 1) 10^q; rounding is monotone, so it is decided only when both ends are decided and
// give the same double.
// q outside the table (-310 .. 345): w >= 1 and q >= 309 is an overflow (inf), w 10^q < 10^(q + 20) <= 1e-325 for
// q <= -345 is an underflow (0); the rest is undecided.  An undecided token is resolved by the caller (the host route of
// chainfiles.loadNumpyTxt converts its bytes with float()): no multi-word path is needed on the device.
#pragma once
#include "fmtdouble.hpp"

#define GD_PARSE_DECIDED 0
#define GD_PARSE_UNDECIDED 1
#define GD_PARSE_NAN_TOKEN 2

namespace gdparse {

typedef unsigned __int128 u128;

// round(w 10^q) for w != 0 and q inside the table; `sign` is the sign bit in place
GD_HD inline int decide(uint64_t w, int q, uint64_t sign, uint64_t* bits) {
    const int lz = gdfmt::clz64(w);
    const uint64_t w64 = w << lz;
    const uint64_t thi = gdfmt::POW10_128[q - GD_FMT_QMIN][0], tlo = gdfmt::POW10_128[q - GD_FMT_QMIN][1];
    const int eT = ((q * 1741647) >> 19) - 127;  // floor(q log2 10) - 127 (checked by the generator script)
    const u128 plo = (u128)w64 * tlo;
    const u128 hi = (u128)w64 * thi + (plo >> 64);  // bits 64..191 of P
    const uint64_t w0 = (uint64_t)plo;              // bits 0..63
    const int top = (int)(hi >> 127);               // n = 190 + top
    const int E = 190 + top + eT - lz;              // floor(log2 of the value) as far as P tells
    int be = E + 1023;                              // biased exponent
    if (be >= 2047) {
        *bits = sign | 0x7ff0000000000000ULL;
        return GD_PARSE_DECIDED;
    }
    int keep = 53;  // bits of P that the result holds
    if (be <= 0) {
        keep = 52 + be;
        be = 1;  // with the hidden bit absent the sum below lands in the subnormal range (or on the least normal)
        if (keep < 0) {  // below 2^-1075, half the least subnormal -- unless the true product carries into the next bit:
            // P + 2^64 passes 2^(n + 1) only when every bit of `hi` up to its top one, bit 126 + top, is set.  (With
            // w >= 1 and q >= GD_FMT_QMIN the value is 1e-310 at the least and keep >= 45: this branch is for soundness.)
            if (keep == -1 && hi == (~(u128)0 >> (1 - top))) return GD_PARSE_UNDECIDED;
            *bits = sign;
            return GD_PARSE_DECIDED;
        }
    }
    const int sh = 127 + top - keep;  // s - 64: bits of `hi` that are dropped, 74 .. 128
    const u128 quo = sh < 128 ? hi >> sh : (u128)0;
    const u128 Rhi = sh < 128 ? hi & (((u128)1 << sh) - 1) : hi;
    const u128 Hhi = (u128)1 << (sh - 1);
    int up;
    if (q >= 0 && q <= 55) {
        up = Rhi > Hhi || (Rhi == Hhi && (w0 != 0 || ((uint64_t)quo & 1u)));
    } else {
        if (Rhi == Hhi - 1) return GD_PARSE_UNDECIDED;
        up = Rhi >= Hhi;
    }
    const uint64_t r = ((uint64_t)(be - 1) << 52) + (uint64_t)quo + (uint64_t)up;  // a carry out of the significand raises the exponent
    *bits = sign | (r >= 0x7ff0000000000000ULL ? 0x7ff0000000000000ULL : r);
    return GD_PARSE_DECIDED;
}

GD_HD inline int lower(int c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }

// One token of `len` bytes read through get(i), i in [0, len).  With VALUE = false only the grammar is checked (the
// verdict is GD_PARSE_DECIDED or GD_PARSE_NAN_TOKEN and *bits is left alone).
template <bool VALUE, class Get>
GD_HD inline int parse_token_with(Get get, int len, uint64_t* bits) {
    int i = 0;
    uint64_t sign = 0;
    if (len <= 0) return GD_PARSE_NAN_TOKEN;
    int c = get(0);
    if (c == '+' || c == '-') {
        sign = c == '-' ? 0x8000000000000000ULL : 0;
        i = 1;
        if (len == 1) return GD_PARSE_NAN_TOKEN;
        c = get(1);
    }
    const int lc = lower(c);
    if (lc == 'n' || lc == 'i') {
        const char* word = lc == 'n' ? "nan" : "infinity";
        const int rest = len - i;
        if (!(rest == 3 || (lc == 'i' && rest == 8))) return GD_PARSE_NAN_TOKEN;
        for (int k = 0; k < rest; ++k)
            if (lower(get(i + k)) != word[k]) return GD_PARSE_NAN_TOKEN;
        if (VALUE) *bits = sign | (lc == 'n' ? 0x7ff8000000000000ULL : 0x7ff0000000000000ULL);
        return GD_PARSE_DECIDED;
    }
    uint64_t w = 0;
    int nd = 0, frac = 0, dropped = 0, any = 0, point = 0, tail = 0;
    for (; i < len; ++i) {
        c = get(i);
        if (c >= '0' && c <= '9') {
            any = 1;
            if (nd < 19) {
                if (w != 0 || c != '0') {
                    w = w * 10u + (uint64_t)(c - '0');
                    ++nd;
                }
                frac += point;
            } else {
                tail |= c != '0';
                dropped += !point;
            }
        } else if (c == '.' && !point) {
            point = 1;
        } else {
            break;
        }
    }
    if (!any) return GD_PARSE_NAN_TOKEN;
    int ex = 0;
    if (i < len) {
        if (c != 'e' && c != 'E') return GD_PARSE_NAN_TOKEN;
        ++i;
        int eneg = 0;
        if (i < len && (get(i) == '+' || get(i) == '-')) {
            eneg = get(i) == '-';
            ++i;
        }
        if (i >= len) return GD_PARSE_NAN_TOKEN;
        for (; i < len; ++i) {
            c = get(i);
            if (c < '0' || c > '9') return GD_PARSE_NAN_TOKEN;
            if (ex < 100000) ex = ex * 10 + (c - '0');
        }
        if (eneg) ex = -ex;
    }
    if (!VALUE) return GD_PARSE_DECIDED;
    if (w == 0) {
        *bits = sign;
        return GD_PARSE_DECIDED;
    }
    const int q = ex - frac + dropped;
    if (q >= 309) {
        *bits = sign | 0x7ff0000000000000ULL;
        return GD_PARSE_DECIDED;
    }
    if (q <= -345) {
        *bits = sign;
        return GD_PARSE_DECIDED;
    }
    if (q < GD_FMT_QMIN) return GD_PARSE_UNDECIDED;
    const int v = decide(w, q, sign, bits);
    if (v != GD_PARSE_DECIDED || !tail) return v;
    uint64_t above;
    if (decide(w + 1, q, sign, &above) != GD_PARSE_DECIDED || above != *bits) return GD_PARSE_UNDECIDED;
    return GD_PARSE_DECIDED;
}

struct PtrGet {
    const unsigned char* p;
    GD_HD int operator()(int i) const { return p[i]; }
};

// The token in the byte range [s, s + len)
GD_HD inline int parse_token(const unsigned char* s, int len, uint64_t* bits) {
    return parse_token_with<true>(PtrGet{s}, len, bits);
}

}  // namespace gdparse
