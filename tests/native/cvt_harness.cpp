// Host harness of getdist_amd/csrc/cvtfloat.hpp: cvt_array() narrows n doubles, given as bit patterns, to fp16, bf16 and fp32.
// With -DCVT_HARNESS_MAIN it is a stand-alone program (built with -fsanitize=address,undefined) that reads the patterns
// from the file argv[1] into a heap block of exactly their size and writes fp16 | bf16 | fp32 results to argv[2].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../getdist_amd/csrc/cvtfloat.hpp"

extern "C" void cvt_array(const uint64_t* bits, int64_t n, uint16_t* f16, uint16_t* bf16, uint32_t* f32) {
    for (int64_t i = 0; i < n; ++i) {
        double x;
        memcpy(&x, bits + i, 8);
        f16[i] = gdcvt::f64_to_f16_bits(x);
        bf16[i] = gdcvt::f64_to_bf16_bits(x);
        const float f = gdcvt::f64_to_f32(x);
        memcpy(f32 + i, &f, 4);
    }
}

#ifdef CVT_HARNESS_MAIN
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    fseek(in, 0, SEEK_END);
    const long bytes = ftell(in);
    fseek(in, 0, SEEK_SET);
    const int64_t n = bytes / 8;
    uint64_t* bits = (uint64_t*)malloc((size_t)n * 8 + 1);
    uint16_t* f16 = (uint16_t*)malloc((size_t)n * 2 + 1);
    uint16_t* bf16 = (uint16_t*)malloc((size_t)n * 2 + 1);
    uint32_t* f32 = (uint32_t*)malloc((size_t)n * 4 + 1);
    if (fread(bits, 8, (size_t)n, in) != (size_t)n) return 4;
    fclose(in);
    cvt_array(bits, n, f16, bf16, f32);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 5;
    fwrite(f16, 2, (size_t)n, out);
    fwrite(bf16, 2, (size_t)n, out);
    fwrite(f32, 4, (size_t)n, out);
    fclose(out);
    free(bits), free(f16), free(bf16), free(f32);
    printf("converted %lld values\n", (long long)n);
    return 0;
}
#endif
