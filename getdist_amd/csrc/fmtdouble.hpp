// printf-exact "%W.Pe" / "%W.PE" of an IEEE double, written so that the SAME source runs inside a HIP kernel (export.hip)
// and in a plain C++ harness (tests/native), where it is held byte for byte to Python's "%W.Pe" % x.  Integer
// arithmetic only -- no floating-point operation, no libm -- so the g++ build and the gfx950 build give the same bytes
// by construction.  P in 0..17, W in 0..32; a value takes at most max(W, P + 8) bytes.
//
// x = m 2^e2 (m < 2^53).  With n = floor(log2 x), kest = floor(n log10 2) is floor(log10 x) or one less, so for
// q = P - kest the scaled value  y = x 10^q  lies in [10^P, 10^(P+2)): its integer part I holds the P + 1 digits wanted
// plus at most one more, which is dropped again (its value joins the rounding).  All that is needed of y is
// (I, h, sticky): the integer part, whether the fraction is >= 1/2, and whether it is neither 0 nor 1/2 exactly.
//
// Fast path (fmt_e_fast): y = m64 * T[q] * 2^-s, m64 = m shifted to 64 bits, T[q] the 128-bit normalised 10^q of
// fmtdouble_pow10.inc, a 192-bit product from three 64 x 64 multiplies.  For 0 <= q <= 55 the table entry is exact and so
// are I, h, sticky, ties included: with P = 8 that is every magnitude from 1e-47 to 1e9.  Elsewhere T[q] is rounded down
// by d < 1, the product is short of the true one by less than m64 < 2^64, and the fraction point sits at bit s >= 127 of
// it: the top 64 fraction bits f are short by less than 2^(64 - (s - 64)) + 1 <= 3 units.  The true fraction is strictly
// above the computed one (d > 0: 10^q has no 128-bit binary form outside 0..55), so (h, sticky = 1) is right unless the
// low 63 bits of f are within 4 of 2^63, i.e. unless y is within 2^-61 below n/2 for an integer n.  Then -- about one
// value in 2^61 of random data, but every exact tie with q < 0, such as 1234567125000.0 at P = 8 -- the caller takes
//
// the slow exact path (fmt_e_slow): a fixed-size multi-word integer of GD_FMT_WS_WORDS 32-bit words.  q >= 0:
// m 5^q (at most 848 bits) shifted by e2 + q; q < 0: m 2^(e2 + q + 1) (at most 1024 bits) divided by 5^-q in short
// divisions by 5^13 with a sticky remainder.  No recursion, no allocation.  The words live in memory the CALLER hands in:
// the kernels pass a per-wave block of LDS and serialise the (rare) lanes that need it, so nothing is indexed in
// registers or spilled to scratch; the host wrapper fmt_e() passes a stack array.
#pragma once
#include <stdint.h>

#ifndef GD_HD
#ifdef __HIPCC__
#define GD_HD __host__ __device__
#else
#define GD_HD
#endif
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define GD_FMT_CONST static __constant__ const
#else
#define GD_FMT_CONST static const
#endif

#define GD_FMT_MAX_PREC 17
#define GD_FMT_MAX_WIDTH 32
#define GD_FMT_WS_WORDS 36

namespace gdfmt {

typedef unsigned __int128 u128;

#define GD_FMT_QMIN (-310)
#define GD_FMT_QMAX 345
GD_FMT_CONST uint64_t POW10_128[GD_FMT_QMAX - GD_FMT_QMIN + 1][2] = {
#include "fmtdouble_pow10.inc"
};

GD_FMT_CONST uint64_t POW10_64[20] = {1ULL, 10ULL, 100ULL, 1000ULL, 10000ULL, 100000ULL, 1000000ULL, 10000000ULL,
                                      100000000ULL, 1000000000ULL, 10000000000ULL, 100000000000ULL, 1000000000000ULL,
                                      10000000000000ULL, 100000000000000ULL, 1000000000000000ULL, 10000000000000000ULL,
                                      100000000000000000ULL, 1000000000000000000ULL, 10000000000000000000ULL};

GD_FMT_CONST uint32_t POW5_32[14] = {1u, 5u, 25u, 125u, 625u, 3125u, 15625u, 78125u, 390625u, 1953125u, 9765625u,
                                     48828125u, 244140625u, 1220703125u};

GD_FMT_CONST char DIGITS2[201] =
    "0001020304050607080910111213141516171819202122232425262728293031323334353637383940414243444546474849"
    "5051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";

GD_HD inline int clz64(uint64_t v) {  // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)v);
#else
    return __builtin_clzll(v);
#endif
}

// what both paths produce: the decimal significand (P + 1 digits, or 0) and exponent, or a non-finite class
struct Decimal {
    uint64_t digits;
    int exp10;
    int kind;  // 0 finite, 1 inf, 2 nan
    int neg;
};

// x = m 2^e2 for a finite non-zero pattern; kest = floor(floor(log2 x) log10 2)
struct Binary {
    uint64_t m;
    int e2, kest;
};

GD_HD inline Binary decompose(uint64_t bits) {
    const int be = (int)((bits >> 52) & 0x7ff);
    const uint64_t fr = bits & 0xfffffffffffffULL;
    Binary b;
    b.m = be ? (fr | (1ULL << 52)) : fr;
    b.e2 = (be ? be : 1) - 1075;
    const int n = 63 - clz64(b.m) + b.e2;
    b.kest = (n * 78913) >> 18;  // floor(n log10 2) for |n| < 1100 (checked by scripts/gen_fmtdouble_table.py)
    return b;
}

// (I, h, sticky) of y -> the rounded P + 1 digits and the decimal exponent; ties to even
GD_HD inline void round_digits(uint64_t I, int h, int sticky, int kest, int prec, Decimal* d) {
    const uint64_t p10 = POW10_64[prec + 1];
    int k = kest, up;
    if (I >= p10) {  // one digit too many: kest was floor(log10 x) - 1
        const unsigned r = (unsigned)(I % 10u);
        I /= 10u;
        k += 1;
        up = r > 5u || (r == 5u && (h || sticky || (I & 1u)));
    } else {
        up = h && (sticky || (I & 1u));
    }
    I += (uint64_t)up;
    if (I == p10) {  // 9.99..9 rounded up: the carry lengthens the exponent, not the digits
        I = POW10_64[prec];
        k += 1;
    }
    d->digits = I;
    d->exp10 = k;
}

// Classifies the pattern; for a finite non-zero value tries the fast path.  Returns 1 when *d is final, 0 when the
// value needs decimal_slow.
GD_HD inline int decimal_fast(uint64_t bits, int prec, Decimal* d) {
    d->neg = (int)(bits >> 63);
    d->digits = 0;
    d->exp10 = 0;
    d->kind = 0;
    const uint64_t mag = bits & 0x7fffffffffffffffULL;
    if (mag >= 0x7ff0000000000000ULL) {
        d->kind = mag > 0x7ff0000000000000ULL ? 2 : 1;
        return 1;
    }
    if (mag == 0) return 1;
    const Binary b = decompose(bits);
    const int q = prec - b.kest;
    const int lz = clz64(b.m);
    const uint64_t m64 = b.m << lz;
    const uint64_t thi = POW10_128[q - GD_FMT_QMIN][0], tlo = POW10_128[q - GD_FMT_QMIN][1];
    const int eT = ((q * 1741647) >> 19) - 127;  // floor(q log2 10) - 127 (checked by the generator script)
    const u128 plo = (u128)m64 * tlo;
    const u128 hi = (u128)m64 * thi + (plo >> 64);  // bits 64..191 of the product
    const uint64_t w0 = (uint64_t)plo;              // bits 0..63
    const int t = -(b.e2 - lz + eT) - 64;           // the fraction point is at bit t of `hi`
    if (t < 63 || t > 127) return 0;                // cannot happen for kest as above; the exact path takes anything
    const uint64_t I = (uint64_t)(hi >> t);
    uint64_t f;
    int restnz;
    if (t >= 64) {
        const int u = t - 64;
        f = (uint64_t)(hi >> u);
        const u128 below = u ? (hi << (128 - u)) : (u128)0;
        restnz = (below != 0) | (w0 != 0);
    } else {
        f = ((uint64_t)hi << 1) | (w0 >> 63);
        restnz = (w0 << 1) != 0;
    }
    const int h = (int)(f >> 63);
    const uint64_t fl = f & 0x7fffffffffffffffULL;
    int sticky;
    if (q >= 0 && q <= 55) {
        sticky = (fl != 0) | restnz;
    } else {
        if (fl >= 0x7ffffffffffffffcULL) return 0;
        sticky = 1;
    }
    round_digits(I, h, sticky, b.kest, prec, d);
    return 1;
}

// ---- the exact path: little-endian 32-bit words in caller-supplied memory ------------------------------------------
GD_HD inline int big_mul32(uint32_t* w, int n, uint32_t f) {
    uint64_t carry = 0;
    for (int i = 0; i < n; ++i) {
        const uint64_t v = (uint64_t)w[i] * f + carry;
        w[i] = (uint32_t)v;
        carry = v >> 32;
    }
    if (carry) w[n++] = (uint32_t)carry;
    return n;
}

// w <- floor(w / f); returns the remainder
GD_HD inline uint32_t big_div32(uint32_t* w, int n, uint32_t f) {
    uint64_t rem = 0;
    for (int i = n - 1; i >= 0; --i) {
        const uint64_t v = (rem << 32) | w[i];
        w[i] = (uint32_t)(v / f);
        rem = v % f;
    }
    return (uint32_t)rem;
}

GD_HD inline uint32_t big_word(const uint32_t* w, int n, int i) { return (i >= 0 && i < n) ? w[i] : 0u; }

// bits [pos, pos + 32) of w
GD_HD inline uint32_t big_bits32(const uint32_t* w, int n, int pos) {
    const int i = pos >> 5, s = pos & 31;
    const uint32_t lo = big_word(w, n, i);
    return s ? (lo >> s) | (big_word(w, n, i + 1) << (32 - s)) : lo;
}

// `ws` holds GD_FMT_WS_WORDS words.  Only for finite non-zero patterns (decimal_fast returned 0).
GD_HD inline void decimal_slow(uint64_t bits, int prec, uint32_t* ws, Decimal* d) {
    const Binary b = decompose(bits);
    const int q = prec - b.kest;
    int n = 2, sticky = 0;
    int sh;  // y = ws 2^-sh after the steps below
    ws[0] = (uint32_t)b.m;
    ws[1] = (uint32_t)(b.m >> 32);
    if (q >= 0) {
        for (int i = q; i > 0; i -= 13) n = big_mul32(ws, n, POW5_32[i >= 13 ? 13 : i]);
        sh = -(b.e2 + q);
    } else {
        const int a = -q;
        const int E = b.e2 - a + 1;  // one spare bit below the integer part: the half bit
        if (E > 0) {                 // ws <- m << E
            const int wsh = E >> 5, bsh = E & 31;
            const uint64_t m = b.m;
            for (int i = 0; i < wsh; ++i) ws[i] = 0;
            ws[wsh] = (uint32_t)(m << bsh);
            ws[wsh + 1] = (uint32_t)((m << bsh) >> 32);
            ws[wsh + 2] = bsh ? (uint32_t)(m >> (64 - bsh)) : 0u;
            n = wsh + 3;
        }
        for (int i = a; i > 0; i -= 13) sticky |= big_div32(ws, n, POW5_32[i >= 13 ? 13 : i]) != 0;
        sh = 1 + (E < 0 ? -E : 0);
    }
    uint64_t I;
    int h = 0;
    if (sh <= 0) {  // an integer below 2^64
        I = ((uint64_t)ws[0] | ((uint64_t)big_word(ws, n, 1) << 32)) << -sh;
    } else {
        I = (uint64_t)big_bits32(ws, n, sh) | ((uint64_t)big_bits32(ws, n, sh + 32) << 32);
        h = (int)((big_word(ws, n, (sh - 1) >> 5) >> ((sh - 1) & 31)) & 1u);
        const int low = sh - 1;  // bits below the half bit
        for (int i = 0; i < (low >> 5) && i < n; ++i) sticky |= ws[i] != 0;
        if (low & 31) sticky |= (big_word(ws, n, low >> 5) & ((1u << (low & 31)) - 1u)) != 0;
    }
    round_digits(I, h, sticky, b.kest, prec, d);
}

// ---- text ----------------------------------------------------------------------------------------------------------
GD_HD inline int text_length(const Decimal& d, int width, int prec) {
    int len;
    if (d.kind)
        len = 3 + (d.kind == 1 && d.neg);
    else
        len = d.neg + 1 + (prec ? prec + 1 : 0) + 2 + ((d.exp10 >= 100 || d.exp10 <= -100) ? 3 : 2);
    return len > width ? len : width;
}

// n decimal digits of v (zero-padded on the left) at p[0 .. n)
GD_HD inline void put_digits(uint32_t v, int n, char* p) {
    while (n >= 2) {
        const uint32_t r = v % 100u;
        v /= 100u;
        p[n - 1] = DIGITS2[2 * r + 1];
        p[n - 2] = DIGITS2[2 * r];
        n -= 2;
    }
    if (n) p[0] = (char)('0' + v % 10u);
}

// Writes text_length(d, width, prec) bytes, right-justified with spaces, and returns that count.
GD_HD inline int put_text(const Decimal& d, int width, int prec, bool upper, char* out) {
    const int total = text_length(d, width, prec);
    int pos = 0;
    if (d.kind) {
        const int len = 3 + (d.kind == 1 && d.neg);
        for (; pos < total - len; ++pos) out[pos] = ' ';
        if (d.kind == 1 && d.neg) out[pos++] = '-';
        const char a = upper ? 'A' : 'a', i = upper ? 'I' : 'i', n = upper ? 'N' : 'n', f = upper ? 'F' : 'f';
        out[pos] = d.kind == 1 ? i : n;
        out[pos + 1] = d.kind == 1 ? n : a;
        out[pos + 2] = d.kind == 1 ? f : n;
        return total;
    }
    const int ex = d.exp10 < 0 ? -d.exp10 : d.exp10;
    const int len = d.neg + 1 + (prec ? prec + 1 : 0) + 2 + (ex >= 100 ? 3 : 2);
    for (; pos < total - len; ++pos) out[pos] = ' ';
    if (d.neg) out[pos++] = '-';
    // the P + 1 digits one byte to the right, then the first one moves in front of the point
    const int nd = prec + 1;
    char* dig = out + pos + 1;
    if (nd > 9) {
        put_digits((uint32_t)(d.digits / 1000000000u), nd - 9, dig);
        put_digits((uint32_t)(d.digits % 1000000000u), 9, dig + nd - 9);
    } else {
        put_digits((uint32_t)d.digits, nd, dig);
    }
    out[pos] = dig[0];
    if (prec) {
        out[pos + 1] = '.';
        pos += 2 + prec;
    } else {
        pos += 1;
    }
    out[pos++] = upper ? 'E' : 'e';
    out[pos++] = d.exp10 < 0 ? '-' : '+';
    if (ex >= 100) {
        out[pos++] = (char)('0' + ex / 100);
        put_digits((uint32_t)(ex % 100), 2, out + pos);
    } else {
        put_digits((uint32_t)ex, 2, out + pos);
    }
    return total;
}

// The fast path alone: the length written, or -1 (nothing written) when the value needs fmt_e_slow.
GD_HD inline int fmt_e_fast(uint64_t bits, int width, int prec, bool upper, char* out) {
    Decimal d;
    if (!decimal_fast(bits, prec, &d)) return -1;
    return put_text(d, width, prec, upper, out);
}

GD_HD inline int fmt_e_slow(uint64_t bits, int width, int prec, bool upper, char* out, uint32_t* ws) {
    Decimal d;
    decimal_fast(bits, prec, &d);  // sign and class
    decimal_slow(bits, prec, ws, &d);
    return put_text(d, width, prec, upper, out);
}

// One value, both paths; `out` has room for max(width, prec + 8) bytes.
GD_HD inline int fmt_e(uint64_t bits, int width, int prec, bool upper, char* out) {
    int len = fmt_e_fast(bits, width, prec, upper, out);
    if (len < 0) {
        uint32_t ws[GD_FMT_WS_WORDS];
        len = fmt_e_slow(bits, width, prec, upper, out, ws);
    }
    return len;
}

}  // namespace gdfmt
