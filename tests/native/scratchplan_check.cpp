// Host check of getdist_amd/csrc/scratchplan.hpp against a stub of the allocation call.  Prints what the plan laid out
// (tests/test_native_scratchplan.py computes the expected layout itself); the modes that use a buffer without a block
// are expected to stop in the header's assert.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../getdist_amd/csrc/scratchplan.hpp"

struct gd_ctx {
    int calls = 0, calls2 = 0;
    int64_t asked = -1;
    bool fail = false;
};
static char g_block[1], g_block2[1];  // never dereferenced: only addresses are compared
void* gd_scratch(gd_ctx* ctx, int64_t bytes) {
    ++ctx->calls, ctx->asked = bytes;
    return ctx->fail ? nullptr : g_block;
}
void* gd_scratch2(gd_ctx* ctx, int64_t bytes) {
    ++ctx->calls2, ctx->asked = bytes;
    return ctx->fail ? nullptr : g_block2;
}

struct Rec24 {
    double a, b, c;
};
static const int64_t kCounts[] = {0, 1, 255, 256, 257, 4096, ((int64_t)1 << 33) + 1};
static const int kN = sizeof(kCounts) / sizeof(kCounts[0]);

// one plan of the seven counts in element type T, then pad(pad_bytes); the second block when `second`
template <class T>
static int layout(const char* name, int64_t pad_bytes, bool second) {
    gd_ctx ctx;
    ScratchPlan sp;
    ScratchPlan::Buf<T> b[kN];
    for (int i = 0; i < kN; ++i) b[i] = sp.take<T>(kCounts[i]);
    sp.pad(pad_bytes);
    const int rc = second ? sp.get2(&ctx) : sp.get(&ctx);
    if (rc != GD_OK || ctx.calls + ctx.calls2 != 1 || (second ? ctx.calls2 : ctx.calls) != 1 || ctx.asked != sp.bytes()) return 1;
    const char* base = second ? g_block2 : g_block;
    for (int i = 0; i < kN; ++i) {
        T* p = b[i];  // the conversion a kernel-launch argument goes through
        if ((const char*)p - base != b[i].off) return 2;
        printf("buf %s %d %lld %lld\n", name, (int)sizeof(T), (long long)kCounts[i], (long long)b[i].off);
    }
    printf("total %s %lld %lld\n", name, (long long)pad_bytes, (long long)sp.bytes());
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "layout";
    if (!strcmp(mode, "layout")) {
        int bad = layout<char>("char", 0, false) | layout<short>("short", 256, true) | layout<int>("int", 512, false) |
                  layout<double>("double", 64, true) | layout<Rec24>("rec24", 0, false);
        {  // 2^31 doubles are 2^34 bytes; a tail is not rounded up and a sub-layout is placed inside another block
            ScratchPlan sp;
            sp.take<double>((int64_t)1 << 31);
            printf("big %lld\n", (long long)sp.bytes());
            ScratchPlan outer, inner;
            auto a = inner.take<int>(3);
            auto t = inner.tail<int>(3);
            auto head = outer.take<char>(1);
            auto sub = outer.tail<char>(inner.bytes());
            gd_ctx ctx;
            bad |= outer.get(&ctx) != GD_OK || inner.place(sub) != GD_OK;
            printf("tail %lld %lld %lld\n", (long long)t.off, (long long)inner.bytes(), (long long)outer.bytes());
            bad |= (char*)(int*)a != g_block + 256 || (char*)(int*)t != g_block + 512 || (char*)head != g_block;
        }
        return bad;
    }
    // the remaining modes end in the assert (or, wrongly, in exit status 0)
    gd_ctx ctx;
    ScratchPlan sp;
    auto a = sp.take<double>(4);
    auto b = sp.take<int>(0);
    if (!strcmp(mode, "fail")) {
        ctx.fail = true;
        const int rc = sp.get(&ctx), rc2 = sp.get2(&ctx);
        printf("rc %d %d\n", rc, rc2);
        fflush(stdout);
        if (argc > 2) {
            int* p = b;  // after the failed allocation: the zero-sized buffer too
            printf("unreachable %p\n", (void*)p);
        } else {
            double* p = a;
            printf("unreachable %p\n", (void*)p);
        }
    } else if (!strcmp(mode, "early")) {
        double* p = a;  // before get()
        printf("unreachable %p\n", (void*)p);
    } else if (!strcmp(mode, "unbound")) {
        ScratchPlan::Buf<double> none;  // a handle no plan has issued
        double* p = none;
        printf("unreachable %p\n", (void*)p);
    }
    return 0;
}
