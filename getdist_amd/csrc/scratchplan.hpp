// The one way an entry point lays out a scratch block (plain C++17, no HIP: compiles with g++ like fft288.hpp).
//
//     ScratchPlan sp;
//     auto d_part = sp.take<double>((int64_t)nblk * 4);   // declare: element type and element count
//     auto d_idx = sp.take<int>(ncols);
//     GD_TRY(sp.get(ctx));                                // one call obtains the block (get2: the second block)
//     k<<<...>>>(d_part, d_idx);                          // a handle converts to its T*
//
// Every buffer starts at the running offset, which then advances by the buffer's bytes rounded up to 256; a buffer of
// 0 elements takes no space and shares the next buffer's offset.  Slack beyond the buffers is said with pad().
// A handle used before get()/get2() succeeded (or after it failed) stops in an assert: it never yields nullptr + offset.
#pragma once
#include <assert.h>
#include <stdint.h>

#include "../../include/gdhip.h"

void* gd_scratch(gd_ctx* ctx, int64_t bytes);  // core.hip: nullptr (and the context's error text set) on failure
void* gd_scratch2(gd_ctx* ctx, int64_t bytes);

struct ScratchPlan {
    template <class T>
    struct Buf {
        const ScratchPlan* plan = nullptr;
        int64_t off = 0;  // from the start of the block
        T* ptr() const {
            assert(plan && plan->base && "scratch buffer used before ScratchPlan::get");
            return (T*)(plan->base + off);
        }
        operator T*() const { return ptr(); }
    };
    ScratchPlan() = default;
    ScratchPlan(const ScratchPlan&) = delete;  // the handles point at their plan
    ScratchPlan& operator=(const ScratchPlan&) = delete;
    template <class T>
    Buf<T> take(int64_t count) {
        const Buf<T> b{this, total};
        total += (count * (int64_t)sizeof(T) + 255) / 256 * 256;
        return b;
    }
    // the last buffer of a block whose end is not rounded up
    template <class T>
    Buf<T> tail(int64_t count) {
        const Buf<T> b{this, total};
        total += count * (int64_t)sizeof(T);
        return b;
    }
    void pad(int64_t bytes) { total += bytes; }
    int64_t bytes() const { return total; }
    int get(gd_ctx* ctx) { return place(gd_scratch(ctx, total)); }
    int get2(gd_ctx* ctx) { return place(gd_scratch2(ctx, total)); }
    // a layout that lives inside another block (a sub-layout shared by a sizing caller and a carving caller)
    int place(void* block) {
        base = (char*)block;
        return base ? GD_OK : GD_ERR_NOMEM;
    }

private:
    int64_t total = 0;
    char* base = nullptr;
};
