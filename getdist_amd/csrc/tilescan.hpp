// Count -> scan -> place, the ordered compaction every variable-length output here is built from: a first pass counts per
// tile (block_sum, ctx.hpp), one block scans the tile counts into offsets (k_tile_scan / gd_tile_offsets), a second pass
// places behind the tile's offset.  The text of export.hip, the rows of ingest.hip, the edges of contourpaths.hip and the
// cumulative weights of thin.hip bring their own passes and share the scan; the ascending row lists of draw.hip and
// select.hip also share the two passes (gd_compact_count / gd_compact_place) and differ in their predicate alone.
#pragma once
#include "ctx.hpp"

// exclusive scan of the nb tile counts in place, 1024 per pass of one block; cnt[nb] receives the total
static __global__ void __launch_bounds__(1024) k_tile_scan(long long* __restrict__ cnt, int nb) {
    __shared__ long long sh[1024];
    __shared__ long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < nb; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const long long v = (i < nb) ? cnt[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const long long a = (threadIdx.x >= (unsigned)o) ? sh[threadIdx.x - o] : 0;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nb) cnt[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[nb] = carry;
}

// Enqueues the scan of cnt[0 .. nb) and, when total_out is given, the fetch of the total cnt[nb]: the caller's next
// gd_stream_sync delivers it.
static inline int gd_tile_offsets(gd_ctx* ctx, long long* cnt, int nb, long long* total_out) {
    k_tile_scan<<<1, 1024, 0, ctx->stream>>>(cnt, nb);
    GD_KERNEL_CHECK();
    if (total_out) GD_TRY(gd_fetch(ctx, total_out, cnt + nb, 8));
    return GD_OK;
}

// Ordered row compaction.  A block owns a tile of THREADS * ITEMS consecutive rows; keep(tile) is evaluated by every
// thread of the block and returns the mask whose bit q says that row  tile * THREADS * ITEMS + q * THREADS + threadIdx.x
// is kept (lane-consecutive rows: coalesced reads).  Both passes evaluate it, so the flags never exist in memory.
template <int THREADS, int ITEMS, class Keep>
__global__ void __launch_bounds__(THREADS) k_compact_count(Keep keep, long long* __restrict__ cnt) {
    __shared__ int red[THREADS / WAVE];
    const int t = block_sum((int)__popc(keep(blockIdx.x)), red);
    if (threadIdx.x == 0) cnt[blockIdx.x] = t;
}

// off: the exclusive scan of the tile counts.  A kept row goes to off[tile] + its rank inside the tile (ballots per wave
// and item round), so the list comes out ascending; nothing is stored at or beyond `capacity`.
template <int THREADS, int ITEMS, class Keep>
__global__ void __launch_bounds__(THREADS)
k_compact_place(Keep keep, const long long* __restrict__ off, int32_t* __restrict__ rows, int64_t capacity) {
    constexpr int WAVES = THREADS / WAVE;
    __shared__ int wave_cnt[ITEMS][WAVES];  // kept rows of (item round, wave): the tile's rows in ascending order
    const unsigned m = keep(blockIdx.x);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int rank[ITEMS];  // kept rows of this round in lower lanes of this wave
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        const unsigned long long b = __ballot((m >> q) & 1u);
        rank[q] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[q][wv] = __popcll(b);
    }
    __syncthreads();
    long long base = off[blockIdx.x];
    const int64_t i0 = (int64_t)blockIdx.x * (THREADS * ITEMS) + threadIdx.x;
#pragma unroll
    for (int q = 0; q < ITEMS; ++q) {
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) {
            const int v = wave_cnt[q][k];
            before += (k < wv) ? v : 0;
            total += v;
        }
        const long long at = base + before + rank[q];
        if (((m >> q) & 1u) && at < capacity) rows[at] = (int32_t)(i0 + (int64_t)q * THREADS);
        base += total;
    }
}

// The two host steps, neither of which waits: count + scan with the fetch of the total enqueued (cnt holds nb + 1
// entries), and place.  A caller that must know the total before it places synchronises between them.
template <int THREADS, int ITEMS, class Keep>
int gd_compact_count(gd_ctx* ctx, const Keep& keep, int nb, long long* cnt, long long* total_out) {
    k_compact_count<THREADS, ITEMS><<<nb, THREADS, 0, ctx->stream>>>(keep, cnt);
    GD_KERNEL_CHECK();
    return gd_tile_offsets(ctx, cnt, nb, total_out);
}
template <int THREADS, int ITEMS, class Keep>
int gd_compact_place(gd_ctx* ctx, const Keep& keep, int nb, const long long* off, int32_t* rows, int64_t capacity) {
    k_compact_place<THREADS, ITEMS><<<nb, THREADS, 0, ctx->stream>>>(keep, off, rows, capacity);
    GD_KERNEL_CHECK();
    return GD_OK;
}
