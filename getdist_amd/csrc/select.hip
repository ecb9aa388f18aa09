// Editing the resident sample set on the device (gd_select_samples, gd_set_weights): the mutators of a sample set (filter,
// thin, removeBurn, deleteFixedParams, addDerived, re-weighting) without the host's fancy indexing and the re-upload.
//
// gd_select_samples builds the new set beside the old one:
//   row list   a mask or a weight threshold becomes an ascending int32 row list (rowlist.hpp).
//   gather     k_sel_gather: out[c][k] = in[col(c)][rows[k]].  A thread owns two consecutive k (one 16-byte store per
//              column), keeps its two row numbers in registers and walks a chunk of GATHER_CH columns with all the chunk's
//              loads in flight before the first store; grid (row tiles, column chunks).  For an ascending list the loads of
//              a wave fall into the lines the kept rows touch, so a dense mask reads about what a streaming compaction
//              would and a sparse one reads less: there is no second, streaming kernel.  The weight column and a host
//              vector to append are separate allocations and go through a second launch of the same kernel.
//   ALL/RANGE  no list: one device-to-device copy per column.
//   install    gd_upload_weight_flags on the new weight column, then the old set is released and the new one installed
//              through the two ends every upload uses.
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "rowlist.hpp"

namespace {

constexpr int GATHER_CH = 8;  // columns per block of the gather

// out[c * ld_out + k] = in[col(c) * ld_in + rows[k]], col(c) = colmap[c] (colmap == nullptr: c), k < K, c < ncols.
// out + c * ld_out is 16-byte aligned for every c (ld_out is a multiple of 512, the base a hipMalloc block).
__global__ void __launch_bounds__(kSelThreads)
k_sel_gather(const double* __restrict__ in, int64_t ld_in, const int32_t* __restrict__ colmap, int ncols,
             const int32_t* __restrict__ rows, int64_t K, double* __restrict__ out, int64_t ld_out) {
    const int64_t k0 = ((int64_t)blockIdx.x * kSelThreads + threadIdx.x) * 2;
    if (k0 >= K) return;
    const bool two = k0 + 1 < K;
    const int64_t ra = rows[k0], rb = two ? rows[k0 + 1] : ra;
    const int c0 = blockIdx.y * GATHER_CH;
    double a[GATHER_CH], b[GATHER_CH];
#pragma unroll
    for (int i = 0; i < GATHER_CH; ++i) {
        const int c = c0 + i;
        if (c < ncols) {
            const double* s = in + (int64_t)(colmap ? colmap[c] : c) * ld_in;
            a[i] = s[ra];
            b[i] = s[rb];
        }
    }
#pragma unroll
    for (int i = 0; i < GATHER_CH; ++i) {
        const int c = c0 + i;
        if (c < ncols) {
            double* d = out + (int64_t)c * ld_out + k0;
            if (two)
                *(double2*)d = make_double2(a[i], b[i]);
            else
                d[0] = a[i];
        }
    }
}

int launch_gather(gd_ctx* ctx, const double* in, int64_t ld_in, const int32_t* d_colmap, int ncols, const int32_t* d_rows, int64_t K,
                  double* out, int64_t ld_out) {
    const int64_t per = 2 * kSelThreads;
    dim3 grid((unsigned)((K + per - 1) / per), (unsigned)((ncols + GATHER_CH - 1) / GATHER_CH));
    k_sel_gather<<<grid, kSelThreads, 0, ctx->stream>>>(in, ld_in, d_colmap, ncols, d_rows, K, out, ld_out);
    GD_KERNEL_CHECK();
    return GD_OK;
}

struct Plan {
    std::vector<int32_t> colmap;  // source column of every new column (the appended spare slot included)
    int m = 0;                    // kept columns
    bool append_host = false;
    bool contiguous = false;      // ALL / RANGE
    int64_t lo = 0, K = 0;        // K: known for ALL / RANGE / ROWS_I32, else found by the scan
};

// fills the new allocations (cols / w / w8 are the caller's locals: it frees them when this fails)
int select_build(gd_ctx* ctx, const gd_selection* sel, const Plan& p, const int32_t* d_rows, const int32_t* d_colmap,
                 double* d_append, int64_t K, int64_t ld, double** cols_out, double** w_out, unsigned char** w8_out, bool* integral_out,
                 double* wsum_out) {
    const int ncols = (int)p.colmap.size(), total = ncols + (p.append_host ? 1 : 0);
    GD_HIP(hipMalloc((void**)cols_out, (size_t)(ld * (total + GD_EXTRA_COLS) * 8)));
    double* cols = *cols_out;
    GD_HIP(hipMemsetAsync(cols + ld * total, 0, (size_t)(ld * GD_EXTRA_COLS * 8), ctx->stream));
    const bool keep_w = sel->weight_kind == GD_SEL_W_KEEP && ctx->w;
    if (keep_w || sel->weight_kind == GD_SEL_W_REPLACE) GD_HIP(hipMalloc((void**)w_out, (size_t)(ld * 8)));
    if (p.contiguous) {
        for (int c = 0; c < ncols; ++c)
            GD_HIP(hipMemcpyAsync(cols + (int64_t)c * ld, ctx->cols + (int64_t)p.colmap[c] * ctx->ld + p.lo, (size_t)(K * 8),
                                  hipMemcpyDeviceToDevice, ctx->stream));
        if (p.append_host)
            GD_HIP(hipMemcpyAsync(cols + (int64_t)ncols * ld, sel->append_host + p.lo, (size_t)(K * 8), hipMemcpyHostToDevice, ctx->stream));
        if (keep_w) GD_HIP(hipMemcpyAsync(*w_out, ctx->w + p.lo, (size_t)(K * 8), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        GD_TRY(launch_gather(ctx, ctx->cols, ctx->ld, d_colmap, ncols, d_rows, K, cols, ld));
        if (p.append_host) {
            GD_HIP(hipMemcpyAsync(d_append, sel->append_host, (size_t)(ctx->N * 8), hipMemcpyHostToDevice, ctx->stream));
            GD_TRY(launch_gather(ctx, d_append, 0, nullptr, 1, d_rows, K, cols + (int64_t)ncols * ld, ld));
        }
        if (keep_w) GD_TRY(launch_gather(ctx, ctx->w, 0, nullptr, 1, d_rows, K, *w_out, ld));
    }
    if (sel->weight_kind == GD_SEL_W_REPLACE)
        GD_HIP(hipMemcpyAsync(*w_out, sel->new_weights, (size_t)(K * 8), hipMemcpyHostToDevice, ctx->stream));
    *integral_out = false;
    *wsum_out = 0;
    if (*w_out) GD_TRY(gd_upload_weight_flags(ctx, *w_out, K, ld, w8_out, integral_out, wsum_out));
    GD_TRY(gd_stream_sync(ctx));
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_select_samples(gd_ctx* ctx, const gd_selection* sel, int64_t* count_out) {
    if (!ctx) return GD_ERR_BADARG;
    GD_REQUIRE(sel, "gd_select_samples: null selection");
    GD_REQUIRE(ctx->cols, "gd_select_samples: no samples uploaded");
    GD_REQUIRE(!ctx->borrowed, "gd_select_samples: the sample set is borrowed (gd_attach_samples): edit it through its owner");
    GD_REQUIRE(ctx->w_sel == 0, "gd_select_samples: auxiliary weights are selected; call gd_select_weights(ctx, 0) first");
    const int64_t N = ctx->N, n = ctx->n;
    GD_REQUIRE(N < 2147483647LL, "gd_select_samples: row indices are 32-bit");
    const bool on_device = (sel->flags & GD_SEL_ROWS_ON_DEVICE) != 0;
    Plan p;
    switch (sel->row_kind) {
        case GD_SEL_ALL:
            p.contiguous = true, p.lo = 0, p.K = N;
            break;
        case GD_SEL_RANGE:
            GD_REQUIRE(sel->lo >= 0 && sel->hi <= N && sel->lo <= N && sel->hi >= 0, "gd_select_samples: row range outside the sample set");
            GD_REQUIRE(sel->lo < sel->hi, "gd_select_samples: no rows selected (empty row range)");
            p.contiguous = true, p.lo = sel->lo, p.K = sel->hi - sel->lo;
            break;
        case GD_SEL_MASK_U8:
            GD_REQUIRE(sel->rows, "gd_select_samples: null row mask");
            break;
        case GD_SEL_WEIGHT_GT:
            GD_REQUIRE(sel->thr == sel->thr, "gd_select_samples: the weight threshold is NaN");
            if (!ctx->w) {  // unit weights: every row or none
                GD_REQUIRE(1.0 > sel->thr, "gd_select_samples: no rows selected");
                p.contiguous = true, p.lo = 0, p.K = N;
            }
            break;
        case GD_SEL_ROWS_I32:
            GD_REQUIRE(sel->K > 0, "gd_select_samples: no rows selected");
            GD_REQUIRE(sel->rows, "gd_select_samples: null row list");
            p.K = sel->K;
            if (!on_device) GD_TRY(check_host_row_list(ctx, "gd_select_samples", (const int32_t*)sel->rows, sel->K, N));
            break;
        default:
            return gd_fail(ctx, GD_ERR_BADARG, "gd_select_samples: unknown row selection %d", (int)sel->row_kind);
    }
    if (sel->keep) {
        GD_REQUIRE(sel->m >= 0, "gd_select_samples: negative column count");
        for (int32_t c = 0; c < sel->m; ++c) {
            GD_REQUIRE(sel->keep[c] >= 0 && sel->keep[c] < n, "gd_select_samples: kept column out of range");
            GD_REQUIRE(c == 0 || sel->keep[c] > sel->keep[c - 1], "gd_select_samples: kept columns must be ascending");
        }
        p.colmap.assign(sel->keep, sel->keep + sel->m);
    } else {
        p.colmap.resize((size_t)n);
        for (int64_t c = 0; c < n; ++c) p.colmap[(size_t)c] = (int32_t)c;
    }
    p.m = (int)p.colmap.size();
    switch (sel->append_kind) {
        case GD_SEL_APPEND_NONE: break;
        case GD_SEL_APPEND_HOST:
            GD_REQUIRE(sel->append_host, "gd_select_samples: null vector to append");
            p.append_host = true;
            break;
        case GD_SEL_APPEND_SLOT:
            GD_REQUIRE(sel->append_slot >= 0 && sel->append_slot < GD_EXTRA_COLS, "gd_select_samples: spare column slot out of range");
            p.colmap.push_back((int32_t)(n + sel->append_slot));
            break;
        default:
            return gd_fail(ctx, GD_ERR_BADARG, "gd_select_samples: unknown append kind %d", (int)sel->append_kind);
    }
    const int64_t total = (int64_t)p.colmap.size() + (p.append_host ? 1 : 0);
    GD_REQUIRE(total > 0, "gd_select_samples: no column left");
    GD_REQUIRE(total <= 65535, "gd_select_samples: more than 65535 resident columns");
    GD_REQUIRE(sel->weight_kind == GD_SEL_W_KEEP || sel->weight_kind == GD_SEL_W_UNIT || sel->weight_kind == GD_SEL_W_REPLACE,
               "gd_select_samples: unknown weight kind");
    if (sel->weight_kind == GD_SEL_W_REPLACE) {
        GD_REQUIRE(sel->new_weights, "gd_select_samples: GD_SEL_W_REPLACE without a weight vector");
        GD_REQUIRE(p.K == 0 || sel->K == p.K, "gd_select_samples: the number of new weights is not the number of rows selected");
    }
    GD_HIP(hipSetDevice(ctx->device));
    GD_TRY(gd_stream_sync(ctx));

    // scratch2: column map | host mask | tile counts | row list | staged vector to append
    const bool scan = !p.contiguous && sel->row_kind != GD_SEL_ROWS_I32;
    const bool host_mask = sel->row_kind == GD_SEL_MASK_U8 && !on_device;
    const bool host_list = sel->row_kind == GD_SEL_ROWS_I32 && !on_device;
    const int nb = (int)((N + GD_SEL_TILE - 1) / GD_SEL_TILE);
    ScratchPlan sp;
    auto b_map = sp.take<int32_t>((int64_t)p.colmap.size());
    auto b_mask = sp.take<unsigned char>(host_mask ? N : 0);
    auto b_cnt = sp.take<long long>(scan ? (int64_t)nb + 1 : 0);
    auto b_rows = sp.take<int32_t>(scan ? N : (host_list ? p.K : 0));
    auto b_app = sp.take<double>(p.append_host && !p.contiguous ? N : 0);
    const int32_t* d_rows = nullptr;
    const int32_t* d_colmap = nullptr;
    double* d_append = nullptr;
    int64_t K = p.K;
    if (!p.contiguous) {
        GD_TRY(sp.get2(ctx));
        d_colmap = b_map;
        d_append = b_app;
        GD_TRY(gd_h2d(ctx, b_map, p.colmap.data(), p.colmap.size() * 4));
        if (scan) {
            const unsigned char* d_mask = nullptr;
            if (sel->row_kind == GD_SEL_MASK_U8) {
                d_mask = (const unsigned char*)sel->rows;
                if (host_mask) {
                    GD_TRY(gd_h2d(ctx, b_mask, sel->rows, (size_t)N));
                    d_mask = b_mask;
                }
            }
            GD_TRY(build_row_list(ctx, d_mask, ctx->w, sel->thr, b_cnt, nb, b_rows, &K));
            d_rows = b_rows;
            GD_REQUIRE(K > 0, "gd_select_samples: no rows selected");
            GD_REQUIRE(sel->weight_kind != GD_SEL_W_REPLACE || sel->K == K,
                       "gd_select_samples: the number of new weights is not the number of rows selected");
        } else if (host_list) {
            GD_TRY(gd_h2d(ctx, b_rows, sel->rows, (size_t)(p.K * 4)));
            d_rows = b_rows;
        } else {
            d_rows = (const int32_t*)sel->rows;
        }
    }
    const int64_t ld = (K + 511) / 512 * 512;
    double *cols = nullptr, *w = nullptr;
    unsigned char* w8 = nullptr;
    bool integral = false;
    double wsum = 0;
    const int rc = select_build(ctx, sel, p, d_rows, d_colmap, d_append, K, ld, &cols, &w, &w8, &integral, &wsum);
    if (rc != GD_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
        if (cols) (void)hipFree(cols);
        if (w) (void)hipFree(w);
        if (w8) (void)hipFree(w8);
        return rc;
    }
    GD_TRY(gd_upload_release(ctx));
    gd_upload_install(ctx, cols, w, w8, integral, wsum, K, total, ld);
    if (count_out) *count_out = K;
    return GD_OK;
}

int gd_set_weights(gd_ctx* ctx, const double* w_host) {
    if (!ctx) return GD_ERR_BADARG;
    GD_REQUIRE(ctx->cols, "gd_set_weights: no samples uploaded");
    GD_REQUIRE(!ctx->borrowed, "gd_set_weights: the sample set is borrowed (gd_attach_samples): edit it through its owner");
    GD_REQUIRE(ctx->w_sel == 0, "gd_set_weights: auxiliary weights are selected; call gd_select_weights(ctx, 0) first");
    GD_HIP(hipSetDevice(ctx->device));
    GD_TRY(gd_stream_sync(ctx));
    double* w = nullptr;
    unsigned char* w8 = nullptr;
    bool integral = false;
    double wsum = 0;
    if (w_host) {
        auto build = [&]() -> int {
            GD_HIP(hipMalloc((void**)&w, (size_t)(ctx->ld * 8)));
            GD_HIP(hipMemcpyAsync(w, w_host, (size_t)(ctx->N * 8), hipMemcpyHostToDevice, ctx->stream));
            GD_TRY(gd_upload_weight_flags(ctx, w, ctx->N, ctx->ld, &w8, &integral, &wsum));
            GD_TRY(gd_stream_sync(ctx));
            return GD_OK;
        };
        const int rc = build();
        if (rc != GD_OK) {  // the previous weights stay
            (void)hipStreamSynchronize(ctx->stream);
            if (w) (void)hipFree(w);
            if (w8) (void)hipFree(w8);
            return rc;
        }
    }
    // everything cached that depends on the weights
    if (ctx->batch_state_release) ctx->batch_state_release(ctx, false);
    if (ctx->w) (void)hipFree(ctx->w);
    if (ctx->w8) (void)hipFree(ctx->w8);
    if (ctx->like_w) (void)hipFree(ctx->like_w);
    if (ctx->wcum) (void)hipFree(ctx->wcum);
    ctx->like_w = ctx->w_main = nullptr;
    ctx->w8_main = nullptr;
    ctx->wcum = nullptr;
    ctx->w_main_sum = 0;
    ctx->w = w;
    ctx->w8 = w8;
    ctx->w_integral = integral;
    ctx->w_sum = wsum;
    ctx->bq = std::make_shared<BucketCols>();  // (16384 buckets with weights, 32768 without: stats.hip)
    return GD_OK;
}

}  // extern "C"
