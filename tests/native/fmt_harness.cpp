// Host build (g++) of getdist_amd/csrc/fmtdouble.hpp for tests/test_fmtdouble_native.py and tests/test_export_cpu.py.
// With -DFMT_HARNESS_MAIN it is a stand-alone program (built with -fsanitize=address,undefined) that formats a fixed set
// of patterns, each into a heap buffer of EXACTLY the documented size max(W, P + 8), and compares with snprintf.
#include "../../getdist_amd/csrc/fmtdouble.hpp"

#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" {

// Formats n bit patterns with "%W.P{e|E}" back to back into `out` (capacity bytes), each followed by `tail` when tail
// >= 0; lens[i] receives the bytes of value i without the tail.  Returns the bytes written, or -1 if they would not fit.
// *slow_count receives how many values left the fast path.
int64_t fmt_array(const uint64_t* bits, int64_t n, int width, int prec, int upper, int tail, char* out, int64_t capacity,
                  int32_t* lens, int64_t* slow_count) {
    const int room = (width > prec + 8 ? width : prec + 8);
    int64_t pos = 0, slow = 0;
    char buf[GD_FMT_MAX_WIDTH + GD_FMT_MAX_PREC + 8];
    uint32_t ws[GD_FMT_WS_WORDS];
    for (int64_t i = 0; i < n; ++i) {
        int len = gdfmt::fmt_e_fast(bits[i], width, prec, upper != 0, buf);
        if (len < 0) {
            ++slow;
            len = gdfmt::fmt_e_slow(bits[i], width, prec, upper != 0, buf, ws);
        }
        if (len > room || pos + len + (tail >= 0) > capacity) return -1;
        memcpy(out + pos, buf, (size_t)len);
        pos += len;
        if (tail >= 0) out[pos++] = (char)tail;
        if (lens) lens[i] = len;
    }
    if (slow_count) *slow_count = slow;
    return pos;
}

// Every value through the exact path (finite non-zero patterns only take it; the others are classified first).
int64_t fmt_array_slow(const uint64_t* bits, int64_t n, int width, int prec, int upper, int tail, char* out,
                       int64_t capacity) {
    int64_t pos = 0;
    char buf[GD_FMT_MAX_WIDTH + GD_FMT_MAX_PREC + 8];
    uint32_t ws[GD_FMT_WS_WORDS];
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t mag = bits[i] & 0x7fffffffffffffffULL;
        const int len = (mag == 0 || mag >= 0x7ff0000000000000ULL) ? gdfmt::fmt_e(bits[i], width, prec, upper != 0, buf)
                                                                   : gdfmt::fmt_e_slow(bits[i], width, prec, upper != 0, buf, ws);
        if (pos + len + (tail >= 0) > capacity) return -1;
        memcpy(out + pos, buf, (size_t)len);
        pos += len;
        if (tail >= 0) out[pos++] = (char)tail;
    }
    return pos;
}

}  // extern "C"

#ifdef FMT_HARNESS_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static uint64_t bits_of(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

static long checked = 0, slow_seen = 0;

// one value into a fresh heap block of exactly max(W, P + 8) bytes: any byte past it is the sanitizer's to report
static int check_one(uint64_t b, int width, int prec, int upper, bool force_slow) {
    const int room = width > prec + 8 ? width : prec + 8;
    char* out = (char*)malloc((size_t)room);
    uint32_t* ws = (uint32_t*)malloc(GD_FMT_WS_WORDS * sizeof(uint32_t));
    const uint64_t mag = b & 0x7fffffffffffffffULL;
    int len = (force_slow && mag != 0 && mag < 0x7ff0000000000000ULL) ? -1 : gdfmt::fmt_e_fast(b, width, prec, upper != 0, out);
    if (len < 0) {
        ++slow_seen;
        len = gdfmt::fmt_e_slow(b, width, prec, upper != 0, out, ws);
    }
    int bad = 0;
    if (mag < 0x7ff0000000000000ULL) {  // glibc agrees with Python on every finite value
        char spec[16], want[64];
        double x;
        memcpy(&x, &b, 8);
        snprintf(spec, sizeof spec, "%%%d.%d%c", width, prec, upper ? 'E' : 'e');
        const int wl = snprintf(want, sizeof want, spec, x);
        if (wl != len || memcmp(want, out, (size_t)len) != 0) {
            fprintf(stderr, "mismatch for %016llx with %s: want '%s' got '%.*s'\n", (unsigned long long)b, spec, want, len, out);
            bad = 1;
        }
    }
    free(ws);
    free(out);
    ++checked;
    return bad;
}

int main() {
    static const int specs[][3] = {{0, 8, 0}, {16, 7, 1}, {15, 7, 1}, {0, 0, 0}, {0, 17, 0}, {25, 16, 0}, {32, 17, 1}};
    const double directed[] = {0.0, -0.0, 1.0, -1.0, 1234567.125, 1234567125000.0, 9.999999995e99, 1e100, 1e-100, 9.999999995e-101,
                               5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 1.7976931348623157e308, 0.5, 1e22, 1e23,
                               123456789.5, 12345678.5, 1e-5, 9.5, 0.95, 8.5, 2.5};
    int bad = 0;
    for (const auto& s : specs) {
        for (double x : directed) {
            const uint64_t b = bits_of(x);
            for (uint64_t nb : {b, b + 1, b ? b - 1 : b, b | ((uint64_t)1 << 63)})
                for (bool slow : {false, true}) bad |= check_one(nb, s[0], s[1], s[2], slow);
        }
        for (uint64_t b : {(uint64_t)0x7ff0000000000000ULL, (uint64_t)0xfff0000000000000ULL, (uint64_t)0x7ff8000000000000ULL, (uint64_t)0xfff8000000000001ULL})
            bad |= check_one(b, s[0], s[1], s[2], false);
        for (int e = -323; e <= 308; ++e) {
            char t[16];
            snprintf(t, sizeof t, "1e%d", e);
            const uint64_t b = bits_of(strtod(t, nullptr));
            for (uint64_t nb : {b - 1, b, b + 1}) bad |= check_one(nb, s[0], s[1], s[2], false), bad |= check_one(nb, s[0], s[1], s[2], true);
        }
    }
    for (int i = 0; i < 200000; ++i) bad |= check_one(next_u64(), 32, 17, i & 1, (i & 7) == 0);
    printf("fmt_harness: %ld values checked, %ld through the exact path, %s\n", checked, slow_seen, bad ? "MISMATCH" : "all equal");
    return bad;
}
#endif
