// Host build (g++) of getdist_amd/csrc/parsedouble.hpp for tests/test_parsedouble_native.py.  With -DPARSE_HARNESS_MAIN it
// is a stand-alone program (built with -fsanitize=address,undefined) that parses a fixed set of tokens, each from a heap
// block of EXACTLY its length, and compares every decided one with glibc's strtod.
#include "../../getdist_amd/csrc/parsedouble.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" {

// The n tokens of `text` (nbytes bytes), one per line ('\n' after every token): bits[i] and verdict[i] of token i.
// Returns the number of tokens seen (== n when the text holds exactly n lines).
int64_t parse_lines(const unsigned char* text, int64_t nbytes, int64_t n, uint64_t* bits, uint8_t* verdict) {
    int64_t k = 0, start = 0;
    for (int64_t i = 0; i < nbytes; ++i) {
        if (text[i] != '\n') continue;
        if (k < n) {
            bits[k] = 0;
            verdict[k] = (uint8_t)gdparse::parse_token(text + start, (int)(i - start), &bits[k]);
        }
        ++k;
        start = i + 1;
    }
    return k;
}

// The grammar check alone (what the scan kernel runs): 1 where the token is a number
int64_t check_lines(const unsigned char* text, int64_t nbytes, int64_t n, uint8_t* ok) {
    int64_t k = 0, start = 0;
    for (int64_t i = 0; i < nbytes; ++i) {
        if (text[i] != '\n') continue;
        if (k < n)
            ok[k] = gdparse::parse_token_with<false>(gdparse::PtrGet{text + start}, (int)(i - start), nullptr) == GD_PARSE_DECIDED;
        ++k;
        start = i + 1;
    }
    return k;
}

}  // extern "C"

#ifdef PARSE_HARNESS_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static long checked = 0, undecided = 0, rejected = 0;

// one token from a fresh heap block of exactly its length: any byte read past it is the sanitizer's to report
static int check_one(const char* tok, bool number) {
    const size_t len = strlen(tok);
    unsigned char* block = (unsigned char*)malloc(len ? len : 1);
    memcpy(block, tok, len);
    uint64_t b = 0;
    const int v = gdparse::parse_token(block, (int)len, &b);
    const int g = gdparse::parse_token_with<false>(gdparse::PtrGet{block}, (int)len, nullptr);
    free(block);
    ++checked;
    int bad = 0;
    if ((g == GD_PARSE_DECIDED) != number || (v == GD_PARSE_NAN_TOKEN) == number) {
        fprintf(stderr, "'%s': verdict %d, grammar %d, expected %s\n", tok, v, g, number ? "a number" : "a rejection");
        return 1;
    }
    if (!number) {
        ++rejected;
        return 0;
    }
    if (v == GD_PARSE_UNDECIDED) {
        ++undecided;
        return 0;
    }
    const double x = strtod(tok, nullptr);
    uint64_t want;
    memcpy(&want, &x, 8);
    if (x != x) want = b;  // NaN patterns are held to Python's by the pytest side
    if (want != b) {
        fprintf(stderr, "'%s': got %016llx, strtod gives %016llx\n", tok, (unsigned long long)b, (unsigned long long)want);
        bad = 1;
    }
    return bad;
}

int main() {
    const char* numbers[] = {"0", "-0", "1.", ".5", "+1", "0.5", ".125", "0e999", "nan", "-NaN", "Infinity", "-inf", "+INF", "1e400",
                             "-1e-400", "5e-324", "4.9406564584124654e-324", "2.4703282292062328e-324", "2.4703282292062329e-324",
                             "1.7976931348623157e308", "1.7976931348623158e308", "1.7976931348623159e308", "9007199254740993",
                             "9007199254740992.5", "9007199254740993.00000000000000000001", "1e22", "1e23", "8.5", "1E+05",
                             "0.000000000000000000000000000000000000012345678901234567890123456789",
                             "123456789012345678901234567890123456789000000000000000000000", "1.00000000000000000000000000000",
                             "2.2250738585072014e-308", "2.2250738585072011e-308", "1e-310", "1e-345", "9e-346", "1e308", "1e309"};
    const char* rejects[] = {"", "1_0", "0x10", "1d5", "1e", "1e+", ".", "+", "-", "1.2.3", "1j", "--1", "e5", ".e5", "na", "infi",
                             "nanx", "infinityy", "1e5.", "1 ", "\xc3\xa9", "1\xff"};
    int bad = 0;
    for (const char* t : numbers) bad |= check_one(t, true);
    for (const char* t : rejects) bad |= check_one(t, false);
    char tok[64];
    for (int i = 0; i < 200000; ++i) {
        const uint64_t b = next_u64();
        double x;
        memcpy(&x, &b, 8);
        if (x != x || x - x != 0) continue;
        static const char* specs[] = {"%.8e", "%16.7E", "%.17e", "%.0e", "%.16g"};
        snprintf(tok, sizeof tok, specs[i % 5], x);
        const char* p = tok;
        while (*p == ' ') ++p;
        bad |= check_one(p, true);
    }
    printf("parse_harness: %ld tokens checked, %ld undecided, %ld rejected, %s\n", checked, undecided, rejected,
           bad ? "MISMATCH" : "all equal");
    return bad;
}
#endif
