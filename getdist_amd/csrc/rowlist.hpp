// The ascending row list of a mask or a weight threshold over the resident sample set, and the check of a host row list:
// what gd_select_samples (select.hip) and gd_export_device (devexport.hip) both select their rows by.  The list is the
// ordered compaction of tilescan.hpp over tiles of GD_SEL_TILE rows with SelKeep as its predicate (count, scan to offsets
// and the total K, place).
#pragma once
#include "ctx.hpp"
#include "tilescan.hpp"

constexpr int kSelThreads = 256;
constexpr int kSelIters = GD_SEL_TILE / kSelThreads;  // rounds of a block over its tile
static_assert(GD_SEL_TILE % kSelThreads == 0, "a tile is a whole number of block rounds");

// the predicate of the compaction (tilescan.hpp): row i is kept when its mask byte is set (mask != nullptr), else when its
// weight exceeds thr
struct SelKeep {
    const unsigned char* mask;
    const double* w;
    double thr;
    int64_t N;

    __device__ __forceinline__ unsigned operator()(int64_t tile) const {
        unsigned m = 0;
#pragma unroll
        for (int q = 0; q < kSelIters; ++q) {
            const int64_t i = tile * GD_SEL_TILE + q * kSelThreads + threadIdx.x;
            if (i < N && (mask ? mask[i] != 0 : w[i] > thr)) m |= 1u << q;
        }
        return m;
    }
};

// the device row list of a mask / threshold selection over the weights `w`, from `d_rows` on (room for N entries; d_cnt:
// one count per tile and one more); K comes back
static inline int build_row_list(gd_ctx* ctx, const unsigned char* d_mask, const double* w, double thr, long long* d_cnt, int nb,
                                 int32_t* d_rows, int64_t* K_out) {
    const SelKeep keep = {d_mask, w, thr, ctx->N};
    long long total = 0;
    GD_TRY((gd_compact_count<kSelThreads, kSelIters>(ctx, keep, nb, d_cnt, &total)));
    GD_TRY((gd_compact_place<kSelThreads, kSelIters>(ctx, keep, nb, d_cnt, d_rows, ctx->N)));  // the list holds N entries
    GD_TRY(gd_stream_sync(ctx));
    *K_out = total;
    return GD_OK;
}

// every entry of a HOST row list lies in [0, N)
static inline int check_host_row_list(gd_ctx* ctx, const char* who, const int32_t* r, int64_t K, int64_t N) {
    for (int64_t k = 0; k < K; ++k)
        if (r[k] < 0 || r[k] >= N)
            return gd_fail(ctx, GD_ERR_BADARG, "%s: row %d (entry %lld of the list) is outside [0, %lld)", who, (int)r[k], (long long)k,
                           (long long)N);
    return GD_OK;
}
