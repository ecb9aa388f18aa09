// Sample sets from arrays that already live in device memory (gd_upload_device), the typed strided read-back the host
// logic needs on that route (gd_fetch_device_array) and the lazy host mirror (gd_download_samples).
//
// gd_upload_device picks one of three kernels per part, from the strides AND the alignment of the pointers:
//   slab    row-major rows (col_stride 1, row_stride close to the column count): a block reads R whole rows as ONE
//           contiguous run with 16-byte loads, keeps them in LDS in the source type, and writes every kept column's R rows
//           as a run of 16-byte stores.  A 32 x 32 tile would leave 14 of 32 lanes idle in its second column tile at n = 50
//           and read 400-byte rows in 256-byte pieces.
//   column  row_stride 1 (column-major, or a vector such as the weights): nothing to transpose, a converting copy per
//           column, two rows per lane where source and destination allow it.
//   tile    anything else (sliced rows, wide row strides, stride 0, a transposed view with gaps): the 32 x 32 LDS tile with
//           strides and a type.  Correct, not fast.
// Wide accesses are used only where the base pointer, the strides and the destination row offset (odd for a chain that
// follows one with an odd row count) make every one of them aligned; otherwise the same kernel runs element-wise.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ctx.hpp"

namespace {

struct f16bits {
    unsigned short b;
};
struct bf16bits {
    unsigned short b;
};
// all three conversions are exact
__device__ __forceinline__ double to_f64(double v) { return v; }
__device__ __forceinline__ double to_f64(float v) { return (double)v; }
__device__ __forceinline__ double to_f64(f16bits v) { return (double)__half2float(__ushort_as_half(v.b)); }
__device__ __forceinline__ double to_f64(bf16bits v) { return (double)__uint_as_float((unsigned int)v.b << 16); }

constexpr int kSlabThreads = 256;
constexpr int kSlabLdsBytes = 64 << 10;  // per block: two blocks of a CU use 128 of its 160 KB

// slab path.  X: the part's first element; the slab of block b is the rs * R elements from X + b * R * rs (the last row of the
// part ends after ncols elements: nothing behind it is read).  LDS keeps element (r, c) at r * pitch + c, pitch odd (in
// elements), so that the column read-out -- lanes a row pair apart -- spreads over the banks.
template <typename T>
__global__ void __launch_bounds__(kSlabThreads)
k_slab_to_cols(const T* __restrict__ X, int64_t rows, int rs, int ncols, int pitch, int rshift, const int* __restrict__ keep, int m,
               double* __restrict__ dst, int64_t ld, int wide_ld, int wide_st) {
    extern __shared__ __align__(16) unsigned char slab_lds[];
    T* lds = (T*)slab_lds;
    const int R = 1 << rshift;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int nr = (int)(rows - r0 < R ? rows - r0 : R);
    const T* slab = X + r0 * rs;
    const int cnt = (nr - 1) * rs + ncols;
    constexpr int V = 16 / (int)sizeof(T);
    const int nv = wide_ld ? cnt / V : 0;
    {
        // (row, column) of this thread's element, advanced by a whole block's worth per round: no division in the loop
        const int first = threadIdx.x * V, step = kSlabThreads * V;
        int r = first / rs, c = first - r * rs;
        const int sr = step / rs, sc = step - sr * rs;
        for (int v = threadIdx.x; v < nv; v += kSlabThreads) {
            union {
                uint4 q;
                T e[V];
            } u;
            u.q = gload_u4(slab + (int64_t)v * V);
            int rr = r, cc = c;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                lds[rr * pitch + cc] = u.e[k];
                if (++cc == rs) cc = 0, ++rr;
            }
            r += sr, c += sc;
            if (c >= rs) c -= rs, ++r;
        }
    }
    {
        const int first = nv * V + threadIdx.x;
        int r = first / rs, c = first - r * rs;
        const int sr = kSlabThreads / rs, sc = kSlabThreads - sr * rs;
        for (int i = first; i < cnt; i += kSlabThreads) {
            lds[r * pitch + c] = slab[i];
            r += sr, c += sc;
            if (c >= rs) c -= rs, ++r;
        }
    }
    __syncthreads();
    const int half = R >> 1;
    for (int item = threadIdx.x; item < m * half; item += kSlabThreads) {
        const int k = item >> (rshift - 1), ra = (item & (half - 1)) * 2;
        if (ra >= nr) continue;
        const int c = keep[k];
        double* d = dst + (int64_t)k * ld + r0 + ra;
        const double a = to_f64(lds[ra * pitch + c]);
        if (ra + 1 < nr) {
            const double b = to_f64(lds[(ra + 1) * pitch + c]);
            if (wide_st) {
                *(double2*)d = make_double2(a, b);
            } else {
                d[0] = a;
                d[1] = b;
            }
        } else {
            d[0] = a;
        }
    }
}

template <typename T>
struct alignas(2 * sizeof(T)) Pair {
    T a, b;
};

// column path: resident column k (blockIdx.y) = source column keep[k] (keep == nullptr: column 0, a vector).
// wide: rs == 1, every column's first element aligned to two elements, dst + k * ld aligned to 16 bytes.
template <typename T>
__global__ void k_cols_copy(const T* __restrict__ X, int64_t rows, int64_t rs, int64_t cs, const int* __restrict__ keep,
                            double* __restrict__ dst, int64_t ld, int wide) {
    const int k = blockIdx.y;
    const T* src = X + (keep ? (int64_t)keep[k] : 0) * cs;
    double* d = dst + (int64_t)k * ld;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    if (wide) {
        const int64_t np = rows >> 1;
        for (int64_t i = t; i < np; i += nt) {
            const Pair<T> p = *(const Pair<T>*)(src + 2 * i);
            *(double2*)(d + 2 * i) = make_double2(to_f64(p.a), to_f64(p.b));
        }
        if ((rows & 1) && t == 0) d[rows - 1] = to_f64(src[rows - 1]);
    } else {
        for (int64_t i = t; i < rows; i += nt) d[i] = to_f64(src[i * rs]);
    }
}

// tile path: resident (row r, column c) = X[r * rs + keep[c] * cs]; writes coalesced, reads as the strides allow
template <typename T>
__global__ void k_tile_to_cols(const T* __restrict__ X, int64_t rows, int64_t rs, int64_t cs, const int* __restrict__ keep, int m,
                               double* __restrict__ dst, int64_t ld) {
    __shared__ double tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        const int64_t r = r0 + k;
        const int c = c0 + threadIdx.x;
        if (r < rows && c < m) tile[k][threadIdx.x] = to_f64(X[r * rs + (int64_t)keep[c] * cs]);
    }
    __syncthreads();
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        const int c = c0 + k;
        const int64_t r = r0 + threadIdx.x;
        if (r < rows && c < m) dst[(int64_t)c * ld + r] = tile[threadIdx.x][k];
    }
}

// rows [r0, r0 + nr) of the described array as row-major fp64 (gd_fetch_device_array)
template <typename T>
__global__ void k_array_to_f64(const T* __restrict__ X, int64_t r0, int64_t nr, int64_t cols, int64_t rs, int64_t cs,
                               double* __restrict__ out) {
    const int64_t total = nr * cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cols, c = i - r * cols;
        out[i] = to_f64(X[(r0 + r) * rs + c * cs]);
    }
}

// resident rows [r0, r0 + nr) of the n columns as row-major fp64 (gd_download_samples): the 32 x 32 tile the other way round
__global__ void k_cols_to_rows(const double* __restrict__ cols, int64_t ld, int64_t r0, int64_t nr, int64_t n,
                               double* __restrict__ out) {
    __shared__ double tile[32][33];
    const int64_t b0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        const int64_t c = c0 + k, r = b0 + threadIdx.x;
        if (r < nr && c < n) tile[k][threadIdx.x] = cols[c * ld + r0 + r];
    }
    __syncthreads();
    for (int k = threadIdx.y; k < 32; k += blockDim.y) {
        const int64_t r = b0 + k, c = c0 + threadIdx.x;
        if (r < nr && c < n) out[r * n + c] = tile[threadIdx.x][k];
    }
}

}  // namespace

// (the three below are shared with devexport.hip: declared in ctx.hpp)
int gd_dtype_bytes(int dtype) {
    switch (dtype) {
        case GD_DT_F64: return 8;
        case GD_DT_F32: return 4;
        case GD_DT_F16:
        case GD_DT_BF16: return 2;
    }
    return 0;
}

// The description (base, shape, strides, element size) names plain device memory of the context's device and stays inside
// its allocation.  Nothing is launched before every array of a call has passed.
int gd_check_device_array(gd_ctx* ctx, const char* what, const void* base, int64_t rows, int64_t cols, int64_t rs, int64_t cs, int sz) {
    if (!base) return gd_fail(ctx, GD_ERR_BADARG, "%s: null pointer", what);
    if (rows <= 0 || cols <= 0) return gd_fail(ctx, GD_ERR_BADARG, "%s: empty shape %lld x %lld", what, (long long)rows, (long long)cols);
    if (rs < 0 || cs < 0)
        return gd_fail(ctx, GD_ERR_DECLINED, "%s: negative stride (%lld, %lld): not served from device memory", what, (long long)rs,
                       (long long)cs);
    if ((uintptr_t)base % (uintptr_t)sz) return gd_fail(ctx, GD_ERR_BADARG, "%s: pointer not aligned to its %d-byte elements", what, sz);
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, base) != hipSuccess) {
        (void)hipGetLastError();
        return gd_fail(ctx, GD_ERR_NOT_DEVICE, "%s: %p is not memory the HIP runtime knows", what, base);
    }
    if (at.isManaged || at.type == hipMemoryTypeManaged) return gd_fail(ctx, GD_ERR_DECLINED, "%s: managed memory", what);
    if (at.type == hipMemoryTypeHost) return gd_fail(ctx, GD_ERR_DECLINED, "%s: page-locked host memory", what);
    if (at.type != hipMemoryTypeDevice) return gd_fail(ctx, GD_ERR_NOT_DEVICE, "%s: not device memory (type %d)", what, (int)at.type);
    if (at.device != ctx->device)
        return gd_fail(ctx, GD_ERR_OTHER_DEVICE, "%s: memory of device %d, the context is on device %d", what, at.device, ctx->device);
    hipDeviceptr_t ab = nullptr;
    size_t asz = 0;
    GD_HIP(hipMemGetAddressRange(&ab, &asz, (hipDeviceptr_t)base));
    const unsigned __int128 last = (unsigned __int128)(rows - 1) * (unsigned __int128)rs + (unsigned __int128)(cols - 1) * (unsigned __int128)cs;
    const unsigned __int128 span = (last + 1) * (unsigned)sz;
    const uintptr_t lo = (uintptr_t)ab, hi = lo + asz, b = (uintptr_t)base;
    if (b < lo || b > hi || span > (unsigned __int128)(hi - b))
        return gd_fail(ctx, GD_ERR_BADARG, "%s: shape and strides reach %s bytes from %p, its allocation ends %zu bytes from it", what,
                       span > (unsigned __int128)UINT64_MAX ? "more than 2^64" : std::to_string((unsigned long long)span).c_str(), base,
                       (size_t)(hi - b));
    return GD_OK;
}

// the context's stream runs behind everything the producer stream has been given so far; the host does not wait
int gd_wait_for_stream(gd_ctx* ctx, void* producer) {
    if (!producer) return GD_OK;
    hipStream_t s = producer == (void*)1 ? (hipStream_t) nullptr : (hipStream_t)producer;  // 1: the legacy default stream
    hipEvent_t ev = nullptr;
    GD_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ev, 0);
    (void)hipEventDestroy(ev);  // (released once the wait that refers to it has completed)
    GD_HIP(e);
    return GD_OK;
}

namespace {

unsigned blocks_for(int64_t items, int per_block, unsigned cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <typename T>
int launch_vector(gd_ctx* ctx, const void* src, int64_t rows, int64_t stride, double* dst) {
    const int wide = stride == 1 && (uintptr_t)src % (2 * sizeof(T)) == 0 && (uintptr_t)dst % 16 == 0;
    k_cols_copy<T><<<dim3(blocks_for(rows, 512, 4096), 1), 256, 0, ctx->stream>>>((const T*)src, rows, stride, 0, nullptr, dst, 0, wide);
    GD_KERNEL_CHECK();
    return GD_OK;
}

// one part into the resident columns, from row `dst` points at
template <typename T>
int launch_part(gd_ctx* ctx, const gd_dev_part& p, const int* d_keep, const std::vector<int32_t>& keep, double* dst, int64_t ld) {
    const int m = (int)keep.size();
    const int64_t rows = p.rows, ncols = p.cols, cs = p.col_stride;
    const int64_t rs = rows == 1 ? (cs == 1 ? ncols : 0) : p.row_stride;  // (the row stride of a single row means nothing)
    const bool dst16 = (uintptr_t)dst % 16 == 0;  // ld is even, so this holds for every column or for none
    if (rs == 1 && rows > 1) {
        bool wide = dst16 && (uintptr_t)p.base % (2 * sizeof(T)) == 0;
        for (int32_t c : keep) wide = wide && ((int64_t)c * cs) % 2 == 0;
        k_cols_copy<T><<<dim3(blocks_for(rows, 512, 1024), (unsigned)m), 256, 0, ctx->stream>>>((const T*)p.base, rows, 1, cs, d_keep, dst,
                                                                                             ld, wide);
        GD_KERNEL_CHECK();
        return GD_OK;
    }
    if (cs == 1 && rs >= ncols && rs <= 2 * (int64_t)m + 8) {
        const int pitch = (int)rs | 1;
        int rshift = 7;  // 128 rows: a wave writes 1 KB of a column per round
        while (rshift >= 3 && ((int64_t)pitch << rshift) * (int64_t)sizeof(T) > kSlabLdsBytes) --rshift;
        if (rshift >= 3) {
            const int R = 1 << rshift;
            // every block's slab starts R * rs elements (a multiple of 16 bytes: R >= 8) behind the previous one's
            const int wide_ld = (uintptr_t)p.base % 16 == 0;
            k_slab_to_cols<T><<<(unsigned)((rows + R - 1) / R), kSlabThreads, (size_t)R * pitch * sizeof(T), ctx->stream>>>(
                (const T*)p.base, rows, (int)rs, (int)ncols, pitch, rshift, d_keep, m, dst, ld, wide_ld, dst16);
            GD_KERNEL_CHECK();
            return GD_OK;
        }
    }
    dim3 grid((unsigned)((rows + 31) / 32), (unsigned)((m + 31) / 32)), block(32, 8);
    k_tile_to_cols<T><<<grid, block, 0, ctx->stream>>>((const T*)p.base, rows, p.row_stride, cs, d_keep, m, dst, ld);
    GD_KERNEL_CHECK();
    return GD_OK;
}

int device_build(gd_ctx* ctx, const gd_dev_part* parts, int nparts, int dtype, int w_dtype, const std::vector<int32_t>& keep,
                 bool weighted, int64_t N, int64_t ld, void* const* producers, int nproducers, double** cols_out, double** w_out, unsigned char** w8_out,
                 bool* integral_out, double* wsum_out) {
    const int64_t m = (int64_t)keep.size();
    for (int k = 0; k < nproducers; ++k) GD_TRY(gd_wait_for_stream(ctx, producers[k]));
    GD_HIP(hipMalloc((void**)cols_out, (size_t)(ld * (m + GD_EXTRA_COLS) * 8)));
    double* cols = *cols_out;
    GD_HIP(hipMemsetAsync(cols + ld * m, 0, (size_t)(ld * GD_EXTRA_COLS * 8), ctx->stream));
    // the kept-column list, in a scratch block large enough for the weight step that follows on the same stream
    ScratchPlan sp;
    auto d_keep = sp.take<int>(m);
    sp.pad(64 << 10);
    GD_TRY(sp.get(ctx));
    GD_TRY(gd_h2d(ctx, d_keep, keep.data(), (size_t)m * 4));
    int64_t at = 0;
    for (int k = 0; k < nparts; ++k) {
        if (parts[k].rows == 0) continue;
#define GD_PART(T) launch_part<T>(ctx, parts[k], d_keep, keep, cols + at, ld)
        switch (dtype) {
            case GD_DT_F64: GD_TRY(GD_PART(double)); break;
            case GD_DT_F32: GD_TRY(GD_PART(float)); break;
            case GD_DT_F16: GD_TRY(GD_PART(f16bits)); break;
            default: GD_TRY(GD_PART(bf16bits)); break;
        }
#undef GD_PART
        at += parts[k].rows;
    }
    *integral_out = false;
    *wsum_out = 0;
    if (weighted) {
        GD_HIP(hipMalloc((void**)w_out, (size_t)(ld * 8)));
        at = 0;
        for (int k = 0; k < nparts; ++k) {
            if (parts[k].rows == 0) continue;
#define GD_VEC(T) launch_vector<T>(ctx, parts[k].weights, parts[k].rows, parts[k].w_stride, *w_out + at)
            switch (w_dtype) {
                case GD_DT_F64: GD_TRY(GD_VEC(double)); break;
                case GD_DT_F32: GD_TRY(GD_VEC(float)); break;
                case GD_DT_F16: GD_TRY(GD_VEC(f16bits)); break;
                default: GD_TRY(GD_VEC(bf16bits)); break;
            }
#undef GD_VEC
            at += parts[k].rows;
        }
        // (the kept-column list is dead by now: the weight step's scratch use is stream-ordered behind the kernels above)
        GD_TRY(gd_upload_weight_flags(ctx, *w_out, N, ld, w8_out, integral_out, wsum_out));
    }
    GD_TRY(gd_stream_sync(ctx));  // the source may be released (or rewritten by its producer) once this returns
    return GD_OK;
}

}  // namespace

extern "C" {

int gd_upload_device(gd_ctx* ctx, const gd_dev_part* parts, int32_t nparts, int32_t dtype, int32_t w_dtype, const int32_t* keep,
                     int32_t m, void* const* producer_streams, int32_t nstreams) {
    if (!ctx) return GD_ERR_BADARG;
    GD_REQUIRE(parts && nparts > 0, "gd_upload_device: no parts");
    GD_REQUIRE(nstreams >= 0 && (nstreams == 0 || producer_streams), "gd_upload_device: bad producer stream list");
    const int sz = gd_dtype_bytes(dtype);
    GD_REQUIRE(sz != 0, "gd_upload_device: unknown sample element type");
    GD_HIP(hipSetDevice(ctx->device));
    const int64_t ncols = parts[0].cols;
    int64_t N = 0;
    bool weighted = false;
    for (int k = 0; k < nparts; ++k) {
        GD_REQUIRE(parts[k].rows >= 0 && parts[k].cols > 0, "gd_upload_device: bad part shape");
        GD_REQUIRE(parts[k].cols == ncols, "gd_upload_device: parts differ in their column count");
        GD_REQUIRE(parts[k].rows == 0 || parts[k].base, "gd_upload_device: null sample pointer");
        N += parts[k].rows;
        weighted = weighted || parts[k].weights != nullptr;
    }
    GD_REQUIRE(N > 0, "gd_upload_device: no rows");
    GD_REQUIRE(ncols < (1 << 30), "gd_upload_device: too many columns");
    const int wsz = gd_dtype_bytes(w_dtype);
    GD_REQUIRE(!weighted || wsz != 0, "gd_upload_device: unknown weight element type");
    std::vector<int32_t> kept;
    if (keep) {
        GD_REQUIRE(m > 0, "gd_upload_device: empty column list");
        kept.assign(keep, keep + m);
        for (int32_t c : kept) GD_REQUIRE(c >= 0 && c < ncols, "gd_upload_device: kept column out of range");
    } else {
        kept.resize((size_t)ncols);
        for (int64_t c = 0; c < ncols; ++c) kept[(size_t)c] = (int32_t)c;
    }
    GD_REQUIRE(kept.size() <= 65535, "gd_upload_device: more than 65535 resident columns");
    for (int k = 0; k < nparts; ++k) {
        const gd_dev_part& p = parts[k];
        if (p.rows == 0) continue;
        GD_REQUIRE(!weighted || p.weights, "gd_upload_device: weights given for some parts only");
        GD_TRY(gd_check_device_array(ctx, "gd_upload_device samples", p.base, p.rows, p.cols, p.row_stride, p.col_stride, sz));
        if (weighted) GD_TRY(gd_check_device_array(ctx, "gd_upload_device weights", p.weights, p.rows, 1, p.w_stride, 0, wsz));
    }
    // validated: from here on the previous sample set is gone
    GD_TRY(gd_upload_release(ctx));
    const int64_t ld = (N + 511) / 512 * 512;
    double *cols = nullptr, *w = nullptr;
    unsigned char* w8 = nullptr;
    bool integral = false;
    double wsum = 0;
    const int rc = device_build(ctx, parts, nparts, dtype, w_dtype, kept, weighted, N, ld, producer_streams, nstreams, &cols, &w, &w8, &integral,
                                &wsum);
    if (rc != GD_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        if (cols) (void)hipFree(cols);
        if (w) (void)hipFree(w);
        if (w8) (void)hipFree(w8);
        return rc;
    }
    gd_upload_install(ctx, cols, w, w8, integral, wsum, N, (int64_t)kept.size(), ld);
    return GD_OK;
}

int gd_fetch_device_array(gd_ctx* ctx, const void* base, int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride,
                          int32_t dtype, void* producer_stream, double* out) {
    if (!ctx) return GD_ERR_BADARG;
    const int sz = gd_dtype_bytes(dtype);
    GD_REQUIRE(sz != 0, "gd_fetch_device_array: unknown element type");
    GD_REQUIRE(out, "gd_fetch_device_array: null destination");
    GD_HIP(hipSetDevice(ctx->device));
    GD_TRY(gd_check_device_array(ctx, "gd_fetch_device_array", base, rows, cols, row_stride, col_stride, sz));
    GD_TRY(gd_wait_for_stream(ctx, producer_stream));
    const int64_t per = std::max<int64_t>(1, ((int64_t)32 << 20) / (cols * 8));  // rows per staged block
    for (int64_t r0 = 0; r0 < rows; r0 += per) {
        const int64_t nr = std::min(per, rows - r0);
        double* stage = (double*)gd_scratch(ctx, nr * cols * 8);
        if (!stage) return GD_ERR_NOMEM;
        const unsigned nb = blocks_for(nr * cols, 256, 4096);
#define GD_ARR(T) k_array_to_f64<T><<<nb, 256, 0, ctx->stream>>>((const T*)base, r0, nr, cols, row_stride, col_stride, stage)
        switch (dtype) {
            case GD_DT_F64: GD_ARR(double); break;
            case GD_DT_F32: GD_ARR(float); break;
            case GD_DT_F16: GD_ARR(f16bits); break;
            default: GD_ARR(bf16bits); break;
        }
#undef GD_ARR
        GD_KERNEL_CHECK();
        GD_TRY(gd_fetch(ctx, out + r0 * cols, stage, (size_t)(nr * cols * 8)));
        GD_TRY(gd_stream_sync(ctx));
    }
    return GD_OK;
}

int gd_pointer_info(gd_ctx* ctx, const void* ptr, int32_t* kind_out, int32_t* device_out) {
    if (!ctx) return GD_ERR_BADARG;
    GD_REQUIRE(ptr && kind_out && device_out, "gd_pointer_info: null argument");
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    *kind_out = GD_PTR_UNKNOWN;
    *device_out = -1;
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return GD_OK;
    }
    if (at.isManaged || at.type == hipMemoryTypeManaged) {
        *kind_out = GD_PTR_MANAGED;
    } else if (at.type == hipMemoryTypeHost) {
        *kind_out = GD_PTR_PINNED;
    } else if (at.type == hipMemoryTypeDevice) {
        *kind_out = GD_PTR_DEVICE;
        *device_out = at.device;
    }
    return GD_OK;
}

int gd_download_samples(gd_ctx* ctx, double* out) {
    if (!ctx) return GD_ERR_BADARG;
    GD_REQUIRE(out, "gd_download_samples: null destination");
    GD_REQUIRE(ctx->cols, "no samples uploaded");
    GD_HIP(hipSetDevice(ctx->device));
    const int64_t N = ctx->N, n = ctx->n;
    const int64_t per = std::max<int64_t>(32, ((int64_t)64 << 20) / (n * 8) / 32 * 32);  // rows per staged block
    double* stage = (double*)gd_scratch(ctx, std::min(per, N) * n * 8);
    if (!stage) return GD_ERR_NOMEM;
    for (int64_t r0 = 0; r0 < N; r0 += per) {
        const int64_t nr = std::min(per, N - r0);
        dim3 grid((unsigned)((nr + 31) / 32), (unsigned)((n + 31) / 32)), block(32, 8);
        k_cols_to_rows<<<grid, block, 0, ctx->stream>>>(ctx->cols, ctx->ld, r0, nr, n, stage);
        GD_KERNEL_CHECK();
        // (stream-ordered: the next block's kernel overwrites the stage only after this copy has read it)
        GD_HIP(hipMemcpyAsync(out + r0 * n, stage, (size_t)(nr * n * 8), hipMemcpyDeviceToHost, ctx->stream));
    }
    GD_TRY(gd_stream_sync(ctx));
    return GD_OK;
}

}  // extern "C"
