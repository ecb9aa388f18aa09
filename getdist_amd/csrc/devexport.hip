// The resident samples as device arrays (gd_export_device): the mirror image of devinput.hip.  Selected rows of selected
// resident columns (fp64, column c at cols + c * ld) are written into the caller's typed, strided device array; the values
// are narrowed with cvtfloat.hpp (one rounding from the double).  gd_export_alloc / _free / _fetch hold a result that
// outlives every context.
//
// One kernel per call, from the strides AND the alignment of the pointers, as on the way in:
//   slab    contiguous rows [lo, lo + K) into a row-major destination (col_stride 1, row_stride >= m).  A block takes R
//           consecutive rows: it reads each listed column's R-row run with 16-byte loads (two rows per lane, lanes along
//           the run) and keeps the CONVERTED values in LDS column by column, element (r, c) at c * pitch + r; then it
//           writes its rows: with row_stride == m they are ONE contiguous run of nr * m elements, written with 16-byte
//           stores, else every row's m elements are written and the gap behind them is not touched.  The read-out walks
//           the columns of a row, lanes `pitch` elements apart: pitch = R + 1 for 8- and 4-byte elements (an odd number of
//           dwords per lane step for fp32, of dword pairs for fp64: a 32-lane group of ds_read_b32 / ds_read_b64 meets
//           every bank once), R + 2 for 2-byte elements (65 dwords per lane step at R = 128; an odd pitch would put lanes
//           2k and 2k + 1 on one bank).  The write-in is lane-contiguous.  R = 128 rows, halved until m * pitch elements fit
//           64 KB (two blocks per CU in 128 of its 160 KB); HBM, not LDS, bounds the kernel: a CU's share of the memory
//           rate is about 13 bytes per clock, an order of magnitude below what either LDS phase moves.
//   column  row_stride 1 (column-major), or a single column of any stride (the weights): nothing to transpose, a converting
//           copy per column, two rows per lane where source and destination allow it.
//   tile    any other strides (a transposed view with gaps, wide column strides): the 32 x 32 LDS tile with strides and a
//           type.  Correct, not fast.
//   gather  any row list: out[k, c] = convert(cols[c][rows[k]]).  A thread owns one k and walks a chunk of GATHER_CH columns
//           with all the chunk's loads in flight before the first store (the register-chunk pattern of k_sel_gather).
// Wide accesses are used only where base, strides, the source offset lo and the block's first element make every one of
// them aligned (an odd lo leaves the column runs 8-byte aligned); otherwise the same kernel runs element-wise.
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "cvtfloat.hpp"
#include "rowlist.hpp"

namespace {

struct f16bits {
    unsigned short b;
};
struct bf16bits {
    unsigned short b;
};
template <typename T>
__device__ __forceinline__ T narrow(double v);
template <>
__device__ __forceinline__ double narrow<double>(double v) {
    return v;
}
template <>
__device__ __forceinline__ float narrow<float>(double v) {
    return gdcvt::f64_to_f32(v);
}
template <>
__device__ __forceinline__ f16bits narrow<f16bits>(double v) {
    return f16bits{gdcvt::f64_to_f16_bits(v)};
}
template <>
__device__ __forceinline__ bf16bits narrow<bf16bits>(double v) {
    return bf16bits{gdcvt::f64_to_bf16_bits(v)};
}

constexpr int kExpThreads = 256;
constexpr int kExpLdsBytes = 64 << 10;
constexpr int GATHER_CH = 8;
constexpr int kSlabInFlight = 4;  // 16-byte loads a thread of the slab kernel has in flight

// the first row of source column c (colmap == nullptr: the one column at `in`, the weights)
__device__ __forceinline__ const double* src_col(const double* in, int64_t ld, const int32_t* colmap, int c) {
    return colmap ? in + (int64_t)colmap[c] * ld : in;
}

// slab path.  out: element (0, 0) of the destination; rs its row stride (>= m), dense: rs == m; wide_ld: lo is even (every
// column run of a block starts 16-byte aligned: the columns do, R is even); wide_st: dense and out 16-byte aligned (a block's
// run starts R * m elements behind the previous one's, a multiple of 16 bytes: R >= 8).
template <typename T>
__global__ void __launch_bounds__(kExpThreads)
k_export_slab(const double* __restrict__ in, int64_t ld, const int32_t* __restrict__ colmap, int m, int64_t lo, int64_t K,
              T* __restrict__ out, int64_t rs, int rshift, int pitch, int wide_ld, int wide_st) {
    extern __shared__ __align__(16) unsigned char slab_lds[];
    T* lds = (T*)slab_lds;
    const int R = 1 << rshift, half = R >> 1;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int nr = (int)(K - r0 < R ? K - r0 : R);
    // kSlabInFlight items per thread and round, all of a round's loads issued before the first conversion
    for (int item0 = threadIdx.x; item0 < m * half; item0 += kExpThreads * kSlabInFlight) {
        double a[kSlabInFlight], b[kSlabInFlight];
#pragma unroll
        for (int u = 0; u < kSlabInFlight; ++u) {
            const int item = item0 + u * kExpThreads;
            const int c = item >> (rshift - 1), ra = (item & (half - 1)) * 2;
            if (item >= m * half || ra >= nr) continue;
            const double* s = src_col(in, ld, colmap, c) + lo + r0 + ra;
            if (ra + 1 >= nr) {
                a[u] = s[0];
            } else if (wide_ld) {
                const double2 v = gload_d2(s);
                a[u] = v.x, b[u] = v.y;
            } else {
                a[u] = s[0], b[u] = s[1];
            }
        }
#pragma unroll
        for (int u = 0; u < kSlabInFlight; ++u) {
            const int item = item0 + u * kExpThreads;
            const int c = item >> (rshift - 1), ra = (item & (half - 1)) * 2;
            if (item >= m * half || ra >= nr) continue;
            T* l = lds + c * pitch + ra;
            l[0] = narrow<T>(a[u]);
            if (ra + 1 < nr) l[1] = narrow<T>(b[u]);
        }
    }
    __syncthreads();
    const int cnt = nr * m;
    if (wide_st) {  // (rs == m: the block's rows are one run)
        T* run = out + r0 * m;
        constexpr int V = 16 / (int)sizeof(T);
        const int nv = cnt / V;
        // (row, column) of this thread's first element, advanced by a whole block's worth per round: no division in the loop
        const int first = threadIdx.x * V, step = kExpThreads * V;
        int r = first / m, c = first - r * m;
        const int sr = step / m, sc = step - sr * m;
        for (int v = threadIdx.x; v < nv; v += kExpThreads) {
            union {
                uint4 q;
                T e[V];
            } u;
            int rr = r, cc = c;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                u.e[k] = lds[cc * pitch + rr];
                if (++cc == m) cc = 0, ++rr;
            }
            *(uint4*)(run + (int64_t)v * V) = u.q;
            r += sr, c += sc;
            if (c >= m) c -= m, ++r;
        }
        const int i = nv * V + threadIdx.x;  // the run's last elements, fewer than V
        if (i < cnt) run[i] = lds[(i % m) * pitch + i / m];
    } else {
        int r = threadIdx.x / m, c = threadIdx.x - r * m;
        const int sr = kExpThreads / m, sc = kExpThreads - sr * m;
        for (int i = threadIdx.x; i < cnt; i += kExpThreads) {
            out[(r0 + r) * rs + c] = lds[c * pitch + r];
            r += sr, c += sc;
            if (c >= m) c -= m, ++r;
        }
    }
}

template <typename T>
struct alignas(2 * sizeof(T)) Pair {
    T a, b;
};

// column path: destination column k (blockIdx.y) starts at out + k * cs, its rows rs apart.
// wide: rs == 1, lo even, every out + k * cs aligned to two elements.
template <typename T>
__global__ void k_export_cols(const double* __restrict__ in, int64_t ld, const int32_t* __restrict__ colmap, int64_t lo, int64_t K,
                              T* __restrict__ out, int64_t rs, int64_t cs, int wide) {
    const int k = blockIdx.y;
    const double* src = src_col(in, ld, colmap, k) + lo;
    T* d = out + (int64_t)k * cs;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    if (wide) {
        const int64_t np = K >> 1;
        for (int64_t i = t; i < np; i += nt) {
            const double2 v = gload_d2(src + 2 * i);
            *(Pair<T>*)(d + 2 * i) = Pair<T>{narrow<T>(v.x), narrow<T>(v.y)};
        }
        if ((K & 1) && t == 0) d[K - 1] = narrow<T>(src[K - 1]);
    } else {
        for (int64_t i = t; i < K; i += nt) d[i * rs] = narrow<T>(src[i]);
    }
}

// tile path: reads coalesced along the columns' rows, writes as the strides allow
template <typename T>
__global__ void k_export_tile(const double* __restrict__ in, int64_t ld, const int32_t* __restrict__ colmap, int m, int64_t lo, int64_t K,
                              T* __restrict__ out, int64_t rs, int64_t cs) {
    __shared__ double tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        const int c = c0 + k;
        const int64_t r = r0 + threadIdx.x;
        if (r < K && c < m) tile[k][threadIdx.x] = src_col(in, ld, colmap, c)[lo + r];
    }
    __syncthreads();
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        const int64_t r = r0 + k;
        const int c = c0 + threadIdx.x;
        if (r < K && c < m) out[r * rs + (int64_t)c * cs] = narrow<T>(tile[threadIdx.x][k]);
    }
}

// gathered path: grid (row tiles, column chunks)
template <typename T>
__global__ void __launch_bounds__(kExpThreads)
k_export_gather(const double* __restrict__ in, int64_t ld, const int32_t* __restrict__ colmap, int m, const int32_t* __restrict__ rows,
                int64_t K, T* __restrict__ out, int64_t rs, int64_t cs) {
    const int64_t k = (int64_t)blockIdx.x * kExpThreads + threadIdx.x;
    if (k >= K) return;
    const int64_t row = rows[k];
    const int c0 = blockIdx.y * GATHER_CH;
    double a[GATHER_CH];
#pragma unroll
    for (int i = 0; i < GATHER_CH; ++i)
        if (c0 + i < m) a[i] = src_col(in, ld, colmap, c0 + i)[row];
    T* d = out + k * rs + (int64_t)c0 * cs;
#pragma unroll
    for (int i = 0; i < GATHER_CH; ++i)
        if (c0 + i < m) d[(int64_t)i * cs] = narrow<T>(a[i]);
}

// the weights of a unit-weight set
template <typename T>
__global__ void k_export_ones(int64_t K, T* __restrict__ out, int64_t rs) {
    const T one = narrow<T>(1.0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K; i += (int64_t)gridDim.x * blockDim.x) out[i * rs] = one;
}

// GD_EXP_ROWS_COLUMN_NZ: the mask bytes of a resident column, for the compaction
__global__ void k_col_nonzero(const double* __restrict__ col, int64_t N, unsigned char* __restrict__ mask) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x)
        mask[i] = col[i] != 0.0 ? 1 : 0;
}

unsigned blocks_for(int64_t items, int per_block, unsigned cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b, b = t;
    }
    return a;
}

// two of the rows x cols elements at base + r * rs + c * cs (rs, cs >= 0) share an address: a * rs == b * cs has a solution
// with 0 <= a < rows, 0 <= b < cols other than a == b == 0; the smallest one is a = cs / g, b = rs / g, g = gcd(rs, cs)
bool elements_overlap(int64_t rows, int64_t cols, int64_t rs, int64_t cs) {
    if (rs == 0 && cs == 0) return rows > 1 || cols > 1;
    const int64_t g = gcd64(rs, cs);
    return cs / g < rows && rs / g < cols;
}

struct Source {
    const double* in;       // nullptr: unit weights
    int64_t ld;
    const int32_t* colmap;  // device; nullptr: the one column at `in`
    int m;
};

struct Dest {
    void* base;
    int64_t rs, cs;
};

template <typename T>
int launch_contiguous(gd_ctx* ctx, const Source& s, int64_t lo, int64_t K, const Dest& d) {
    T* out = (T*)d.base;
    const int m = s.m;
    if (!s.in) {
        k_export_ones<T><<<blocks_for(K, 256, 4096), 256, 0, ctx->stream>>>(K, out, d.rs);
        GD_KERNEL_CHECK();
        return GD_OK;
    }
    const bool lo_even = (lo & 1) == 0;  // the columns (ld even) and the weight block start 16-byte aligned
    if (m == 1 || (d.rs == 1 && K > 1)) {
        const int64_t rs = K == 1 ? 1 : d.rs;  // (the row stride of a single row means nothing)
        const bool wide = rs == 1 && lo_even && (uintptr_t)out % (2 * sizeof(T)) == 0 && (m == 1 || d.cs % 2 == 0);
        k_export_cols<T><<<dim3(blocks_for(K, 512, 1024), (unsigned)m), 256, 0, ctx->stream>>>(s.in, s.ld, s.colmap, lo, K, out, rs, d.cs, wide);
        GD_KERNEL_CHECK();
        return GD_OK;
    }
    if (d.cs == 1 && (d.rs >= m || K == 1)) {
        const int64_t rs = K == 1 ? m : d.rs;
        int rshift = 7;  // 128 rows: a lane group reads 1 KB of a column per round
        auto pitch_of = [](int shift) { return (1 << shift) + (sizeof(T) == 2 ? 2 : 1); };
        while (rshift >= 3 && (int64_t)m * pitch_of(rshift) * (int64_t)sizeof(T) > kExpLdsBytes) --rshift;
        if (rshift >= 3) {
            const int R = 1 << rshift, pitch = pitch_of(rshift);
            const int wide_st = rs == m && (uintptr_t)out % 16 == 0;
            k_export_slab<T><<<(unsigned)((K + R - 1) / R), kExpThreads, (size_t)m * pitch * sizeof(T), ctx->stream>>>(
                s.in, s.ld, s.colmap, m, lo, K, out, rs, rshift, pitch, lo_even, wide_st);
            GD_KERNEL_CHECK();
            return GD_OK;
        }
    }
    dim3 grid((unsigned)((K + 31) / 32), (unsigned)((m + 31) / 32)), block(32, 8);
    k_export_tile<T><<<grid, block, 0, ctx->stream>>>(s.in, s.ld, s.colmap, m, lo, K, out, d.rs, d.cs);
    GD_KERNEL_CHECK();
    return GD_OK;
}

template <typename T>
int launch_gathered(gd_ctx* ctx, const Source& s, const int32_t* d_rows, int64_t K, const Dest& d) {
    T* out = (T*)d.base;
    if (!s.in) {
        k_export_ones<T><<<blocks_for(K, 256, 4096), 256, 0, ctx->stream>>>(K, out, d.rs);
    } else {
        dim3 grid((unsigned)((K + kExpThreads - 1) / kExpThreads), (unsigned)((s.m + GATHER_CH - 1) / GATHER_CH));
        k_export_gather<T><<<grid, kExpThreads, 0, ctx->stream>>>(s.in, s.ld, s.colmap, s.m, d_rows, K, out, d.rs, d.cs);
    }
    GD_KERNEL_CHECK();
    return GD_OK;
}

// the consumer stream runs behind everything the context's stream has been given so far; the host does not wait
int release_to_stream(gd_ctx* ctx, void* consumer) {
    hipStream_t s = consumer == (void*)1 ? (hipStream_t) nullptr : (hipStream_t)consumer;  // 1: the legacy default stream
    hipEvent_t ev = nullptr;
    GD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, ev, 0);
    (void)hipEventDestroy(ev);  // (released once the wait that refers to it has completed)
    GD_HIP(e);
    return GD_OK;
}

int more_rows(gd_ctx* ctx, int64_t capacity, int64_t K) {
    gd_fail(ctx, GD_DRAW_MORE_ROWS, "gd_export_device: the destination holds %lld rows, the selection has %lld", (long long)capacity,
            (long long)K);
    return GD_DRAW_MORE_ROWS;
}

}  // namespace

extern "C" {

int gd_export_device(gd_ctx* ctx, const gd_export* ex, int64_t* count_out) {
    if (!ctx) return GD_ERR_BADARG;
    GD_REQUIRE(ex && count_out, "gd_export_device: null argument");
    GD_REQUIRE(ctx->cols, "gd_export_device: no samples uploaded");
    const int64_t N = ctx->N, n = ctx->n;
    const bool on_device = (ex->flags & GD_SEL_ROWS_ON_DEVICE) != 0;
    const double* sw = ctx->w_sel ? ctx->w_main : ctx->w;  // always the sample weights
    bool contiguous = false, scan = false;
    int64_t lo = 0, K = 0;
    switch (ex->row_kind) {
        case GD_SEL_ALL:
            contiguous = true, K = N;
            break;
        case GD_SEL_RANGE:
            GD_REQUIRE(ex->lo >= 0 && ex->hi <= N && ex->lo <= ex->hi, "gd_export_device: row range outside the sample set");
            contiguous = true, lo = ex->lo, K = ex->hi - ex->lo;
            break;
        case GD_SEL_MASK_U8:
            GD_REQUIRE(ex->rows, "gd_export_device: null row mask");
            scan = true;
            break;
        case GD_SEL_WEIGHT_GT:
            GD_REQUIRE(ex->thr == ex->thr, "gd_export_device: the weight threshold is NaN");
            if (!sw)  // unit weights: every row or none
                contiguous = true, K = 1.0 > ex->thr ? N : 0;
            else
                scan = true;
            break;
        case GD_SEL_ROWS_I32:
            GD_REQUIRE(ex->K >= 0, "gd_export_device: negative row list length");
            GD_REQUIRE(ex->K == 0 || ex->rows, "gd_export_device: null row list");
            K = ex->K;
            if (!on_device) GD_TRY(check_host_row_list(ctx, "gd_export_device", (const int32_t*)ex->rows, K, N));
            break;
        case GD_EXP_ROWS_COLUMN_NZ:
            GD_REQUIRE(ex->mask_col >= 0 && ex->mask_col < n + GD_EXTRA_COLS, "gd_export_device: mask column out of range");
            scan = true;
            break;
        default:
            return gd_fail(ctx, GD_ERR_BADARG, "gd_export_device: unknown row selection %d", (int)ex->row_kind);
    }
    GD_REQUIRE(contiguous || N < 2147483647LL, "gd_export_device: row indices are 32-bit");
    int m = 1;
    if (ex->cols) {
        GD_REQUIRE(ex->m >= 1 && ex->m <= 65535, "gd_export_device: the column count must be 1 .. 65535");
        GD_REQUIRE_COLUMNS(ex->cols, ex->m);
        m = ex->m;
    }
    const int sz = gd_dtype_bytes(ex->dtype);
    GD_REQUIRE(sz != 0, "gd_export_device: unknown element type");
    const int64_t cap = ex->rows_capacity;
    GD_REQUIRE(cap >= 0, "gd_export_device: negative rows_capacity");
    GD_HIP(hipSetDevice(ctx->device));
    if (cap > 0) {
        GD_TRY(gd_check_device_array(ctx, "gd_export_device destination", ex->base, cap, m, ex->row_stride, ex->col_stride, sz));
        if (elements_overlap(cap, m, ex->row_stride, ex->col_stride))
            return gd_fail(ctx, GD_ERR_BADARG, "gd_export_device: elements of the %lld x %d destination share an address (strides %lld, %lld)",
                           (long long)cap, m, (long long)ex->row_stride, (long long)ex->col_stride);
    }
    if (!scan) {
        *count_out = K;
        if (K > cap) return more_rows(ctx, cap, K);
        if (K == 0) return GD_OK;
    }

    // scratch2: column map | host mask or the mask of a column | tile counts | row list
    const bool host_mask = ex->row_kind == GD_SEL_MASK_U8 && !on_device;
    const bool col_mask = ex->row_kind == GD_EXP_ROWS_COLUMN_NZ;
    const bool host_list = ex->row_kind == GD_SEL_ROWS_I32 && !on_device;
    const int nb = (int)((N + GD_SEL_TILE - 1) / GD_SEL_TILE);
    ScratchPlan sp;
    auto b_map = sp.take<int32_t>(ex->cols ? m : 0);
    auto b_mask = sp.take<unsigned char>(host_mask || col_mask ? N : 0);
    auto b_cnt = sp.take<long long>(scan ? (int64_t)nb + 1 : 0);
    auto b_rows = sp.take<int32_t>(scan ? N : (host_list ? K : 0));
    sp.pad(256);
    GD_TRY(sp.get2(ctx));
    const int32_t* d_rows = nullptr;
    if (scan) {
        const unsigned char* d_mask = nullptr;
        if (ex->row_kind == GD_SEL_MASK_U8) {
            d_mask = (const unsigned char*)ex->rows;
            if (host_mask) {
                GD_TRY(gd_h2d(ctx, b_mask, ex->rows, (size_t)N));
                d_mask = b_mask;
            }
        } else if (col_mask) {
            k_col_nonzero<<<blocks_for(N, 256, 4096), 256, 0, ctx->stream>>>(ctx->cols + (int64_t)ex->mask_col * ctx->ld, N, b_mask);
            GD_KERNEL_CHECK();
            d_mask = b_mask;
        }
        GD_TRY(build_row_list(ctx, d_mask, sw, ex->thr, b_cnt, nb, b_rows, &K));
        d_rows = b_rows;
        *count_out = K;
        if (K > cap) return more_rows(ctx, cap, K);
        if (K == 0) return GD_OK;
    } else if (host_list) {
        GD_TRY(gd_h2d(ctx, b_rows, ex->rows, (size_t)(K * 4)));
        d_rows = b_rows;
    } else if (!contiguous) {
        d_rows = (const int32_t*)ex->rows;
    }
    Source s = {ex->cols ? ctx->cols : sw, ex->cols ? ctx->ld : 0, nullptr, m};
    if (ex->cols) {
        GD_TRY(gd_h2d(ctx, b_map, ex->cols, (size_t)m * 4));
        s.colmap = b_map;
    }
    const Dest d = {ex->base, ex->row_stride, ex->col_stride};
    // the destination may still be in use on the consumer's stream: its earlier work first (the row list above did not
    // touch the destination, and its host wait was for the library's own stream alone)
    GD_TRY(gd_wait_for_stream(ctx, ex->consumer_stream));
#define GD_EXPORT(T) (contiguous ? launch_contiguous<T>(ctx, s, lo, K, d) : launch_gathered<T>(ctx, s, d_rows, K, d))
    switch (ex->dtype) {
        case GD_DT_F64: GD_TRY(GD_EXPORT(double)); break;
        case GD_DT_F32: GD_TRY(GD_EXPORT(float)); break;
        case GD_DT_F16: GD_TRY(GD_EXPORT(f16bits)); break;
        default: GD_TRY(GD_EXPORT(bf16bits)); break;
    }
#undef GD_EXPORT
    if (ex->consumer_stream) return release_to_stream(ctx, ex->consumer_stream);
    return gd_stream_sync(ctx);
}

int gd_export_alloc(int32_t device, int64_t bytes, void** d_out) {
    if (!d_out || bytes < 0) return GD_ERR_BADARG;
    *d_out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return GD_ERR_HIP;
    const hipError_t e = hipMalloc(d_out, (size_t)std::max<int64_t>(bytes, 16));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? GD_ERR_NOMEM : GD_ERR_HIP;
    }
    return GD_OK;
}

int gd_export_free(int32_t device, void* d_ptr) {
    if (!d_ptr) return GD_OK;
    if (hipSetDevice(device) != hipSuccess) return GD_ERR_HIP;
    return hipFree(d_ptr) == hipSuccess ? GD_OK : GD_ERR_HIP;
}

int gd_export_fetch(int32_t device, void* dst, const void* d_src, int64_t bytes) {
    if (bytes <= 0) return GD_OK;
    if (!dst || !d_src) return GD_ERR_BADARG;
    if (hipSetDevice(device) != hipSuccess) return GD_ERR_HIP;
    return hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess ? GD_OK : GD_ERR_HIP;
}

}  // extern "C"
