// Weight-one sample draws (mcsamples.py:578-606 makeSingleSamples; chains.py:918-939 random_single_samples_indices):
// row i is kept when  rand_i <= w_i / (max_weight * thin),  rand = np.random.default_rng(random_state).random(numrows).
//
// The draw is bit-equal to the reference's for the same random_state: numpy's default bit generator is PCG64, whose LCG
// state jumps ahead in O(log n) (pcg64.hpp), so a thread starts at its own row and rand never exists as a vector -- the
// count pass and the write pass each regenerate it.  A generator that is not PCG64 draws on the host and the same two
// kernels read the uploaded vector instead.
//
// The row list is the ordered compaction of tilescan.hpp with DrawArgs as its predicate: a block owns a tile of DRAW_TILE
// consecutive rows and its threads walk it strided (lane-consecutive rows: coalesced weight reads, one multiply-add of the
// 256-step map per row), once in the count pass and once in the place pass.  The list comes out ascending, as np.nonzero
// gives it.
#include "ctx.hpp"
#include "pcg64.hpp"
#include "tilescan.hpp"

#define DRAW_THREADS 256
#define DRAW_ITEMS 8
#define DRAW_TILE (DRAW_THREADS * DRAW_ITEMS)

namespace {
// the predicate of the compaction (tilescan.hpp)
struct DrawArgs {
    const double* w;     // sample weights, nullptr = unit weights
    const double* rand;  // N variates, nullptr = PCG64 from (state, inc)
    int64_t N;
    uint64_t state_hi, state_lo, inc_hi, inc_lo;  // bit_generator.state["state"]
    uint64_t a_hi, a_lo, c_hi, c_lo;              // gdpcg::stride(inc, DRAW_THREADS)
    double a, b;
    int mode;  // 0: w / (a * b)   1: (w / a) / b   -- the reference's two operation orders round differently

    // bit q = this thread's row  tile * DRAW_TILE + q * DRAW_THREADS + threadIdx.x  is kept
    __device__ __forceinline__ unsigned operator()(int64_t tile) const {
        const double ab = a * b;
        int64_t i = tile * DRAW_TILE + threadIdx.x;
        gdpcg::u128 s = 0;
        const gdpcg::Affine step = {gdpcg::make_u128(a_hi, a_lo), gdpcg::make_u128(c_hi, c_lo)};
        if (!rand && i < N) {
            gdpcg::Pcg64 g = {gdpcg::make_u128(state_hi, state_lo), gdpcg::make_u128(inc_hi, inc_lo)};
            g.advance((gdpcg::u128)(uint64_t)(i + 1));  // draw i is the output of the state after i + 1 steps
            s = g.state;
        }
        unsigned m = 0;
#pragma unroll
        for (int q = 0; q < DRAW_ITEMS; ++q, i += DRAW_THREADS) {
            if (i < N) {
                const double r = rand ? rand[i] : gdpcg::to_double(gdpcg::output(s));
                const double wi = w ? w[i] : 1.0;
                const double thr = mode ? (wi / a) / b : wi / ab;
                if (r <= thr) m |= 1u << q;
            }
            s = step(s);
        }
        return m;
    }
};
}  // namespace

// out[k * m + c] = column colidx[c] at row rows[k]; a row outside the sample set gives NaN (never an out-of-range read)
__global__ void __launch_bounds__(256) k_gather_rows(const double* __restrict__ cols, int64_t ld, int64_t N,
                                                     const int32_t* __restrict__ rows, int64_t K,
                                                     const int32_t* __restrict__ colidx, int m, double* __restrict__ out) {
    const int64_t total = K * m;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / m;
        const int c = (int)(e - k * m);
        const int64_t r = rows[k];
        out[e] = (r >= 0 && r < N) ? cols[(int64_t)colidx[c] * ld + r] : __longlong_as_double(0x7ff8000000000000LL);
    }
}

extern "C" {

int gd_draw_single_rows(gd_ctx* ctx, const uint64_t* pcg_state, const void* d_rand, double a, double b, int32_t mode,
                        void* d_rows, int64_t capacity, int64_t* count_out) {
    GD_REQUIRE(ctx && count_out, "null argument");
    GD_REQUIRE(ctx->cols && ctx->N > 0, "no samples uploaded");
    GD_REQUIRE((pcg_state != nullptr) != (d_rand != nullptr), "give the PCG64 state or a vector of variates, not both");
    GD_REQUIRE(mode == 0 || mode == 1, "threshold mode is 0 or 1");
    GD_REQUIRE(capacity >= 0 && (d_rows || capacity == 0), "bad row buffer");
    GD_REQUIRE(ctx->N < 2147483648LL, "row indices are 32-bit");
    const int64_t N = ctx->N;
    const int nb = (int)((N + DRAW_TILE - 1) / DRAW_TILE);
    long long* cnt = (long long*)gd_scratch(ctx, ((int64_t)nb + 1) * 8);
    if (!cnt) return GD_ERR_NOMEM;
    DrawArgs p = {};
    p.w = ctx->w_sel ? ctx->w_main : ctx->w;  // always the sample weights
    p.rand = (const double*)d_rand;
    p.N = N;
    if (pcg_state) {
        const gdpcg::u128 inc = gdpcg::make_u128(pcg_state[2], pcg_state[3]);
        const gdpcg::Affine step = gdpcg::stride(inc, DRAW_THREADS);
        p.state_hi = pcg_state[0], p.state_lo = pcg_state[1], p.inc_hi = pcg_state[2], p.inc_lo = pcg_state[3];
        p.a_hi = gdpcg::hi64(step.a), p.a_lo = gdpcg::lo64(step.a), p.c_hi = gdpcg::hi64(step.c), p.c_lo = gdpcg::lo64(step.c);
    }
    p.a = a, p.b = b, p.mode = mode;
    long long total = 0;
    GD_TRY((gd_compact_count<DRAW_THREADS, DRAW_ITEMS>(ctx, p, nb, cnt, &total)));
    GD_TRY(gd_stream_sync(ctx));
    *count_out = total;
    if (total > capacity) {
        gd_fail(ctx, GD_DRAW_MORE_ROWS, "row buffer holds %lld rows, the draw keeps %lld", (long long)capacity, total);
        return GD_DRAW_MORE_ROWS;
    }
    if (total == 0) return GD_OK;
    GD_TRY((gd_compact_place<DRAW_THREADS, DRAW_ITEMS>(ctx, p, nb, cnt, (int32_t*)d_rows, capacity)));
    GD_TRY(gd_stream_sync(ctx));
    return GD_OK;
}

int gd_gather_rows(gd_ctx* ctx, const void* d_rows, int64_t K, const int32_t* cols, int32_t m, void* d_out) {
    GD_REQUIRE(ctx && cols && m > 0 && K >= 0, "bad argument");
    GD_REQUIRE(ctx->cols, "no samples uploaded");
    for (int i = 0; i < m; ++i) GD_REQUIRE(cols[i] >= 0 && cols[i] < ctx->n + GD_EXTRA_COLS, "column out of range");
    if (K == 0) return GD_OK;
    GD_REQUIRE(d_rows && d_out, "null argument");
    int32_t* d_idx = (int32_t*)gd_scratch(ctx, (int64_t)m * 4);
    if (!d_idx) return GD_ERR_NOMEM;
    GD_TRY(gd_h2d(ctx, d_idx, cols, (size_t)m * 4));
    int64_t nblk = (K * m + 255) / 256;
    if (nblk > 2048) nblk = 2048;
    k_gather_rows<<<(int)nblk, 256, 0, ctx->stream>>>(ctx->cols, ctx->ld, ctx->N, (const int32_t*)d_rows, K, d_idx, m,
                                                     (double*)d_out);
    GD_KERNEL_CHECK();
    GD_TRY(gd_stream_sync(ctx));
    return GD_OK;
}

}  // extern "C"
