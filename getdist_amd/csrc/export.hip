// Chain export (chains.py:1063-1085 saveAsText = np.savetxt(fmt="%.8e"); mcsamples.py:596-601, the "%16.7E" rows of
// makeSingleSamples): sample rows, or a matrix, as text whose bytes equal Python's "%W.Pe" % x (fmtdouble.hpp).
//
// The samples are column-major and the text is row-major, so a block owns a tile of TR consecutive output rows and
// transposes through LDS: thread t takes row t % TR and the fields t / TR, t / TR + 256 / TR, ... (lanes run along rows
// while a column is read: coalesced 8-byte loads), formats each value into a fixed slot, the lengths are summed per
// row and scanned over the tile, the fields are packed back to back in a second LDS block laid out at the alignment of
// the tile's place in the output, and that block goes out in 16-byte stores with lanes on consecutive addresses.
// TR is the largest power of two up to 64 whose tile fits 64 KB of LDS (32 rows for 52 fields of "%.8e").
//
// Rows vary in length (a sign, a three-digit exponent), so a tile needs its byte offset: pass 1 formats every value for
// its length only and writes one count per tile, one block scans the counts (tilescan.hpp), pass 2 formats again and writes.  The text
// is formatted twice rather than kept (it is 2 x the samples' size) or placed by decoupled look-back (which needs
// forward progress between blocks and device-scope ordering for a second read of 8 bytes per value): DESIGN.md gives
// the measured kernel time against the copy of the same text to the host.
//
// A value the formatter's fast path cannot decide (fmtdouble.hpp) takes the exact multi-word path, whose words live in
// a 144-byte LDS block per wave: the lanes that need it run one after the other.
#include "ctx.hpp"
#include "fmtdouble.hpp"
#include "tilescan.hpp"

#define FMT_THREADS 256
#define FMT_WAVES (FMT_THREADS / WAVE)
#define FMT_MAX_TILE_ROWS 64
#define FMT_LDS_BYTES 65536
#define FMT_COUNT_LDS (32 + FMT_WAVES * GD_FMT_WS_WORDS * 4)

struct FmtArgs {
    // gd_format_rows: the resident sample set and the field sources (device copy)
    const double* cols;
    const double* w;
    int64_t ld, N;
    const int32_t* srcs;  // nullptr: gd_format_matrix
    const int32_t* rows;  // nullptr: rows row_lo, row_lo + 1, ...
    int64_t row_lo;
    // gd_format_matrix
    const double* x;
    int64_t rs, cs;
    int64_t K;  // output rows
    int m, width, prec, upper, sep;
    int TR, slot;  // rows per tile, bytes per slot = max(width, prec + 8) + 1
};

// LDS carve (dynamic region only, every offset a multiple of 16)
struct FmtLds {
    int slots, packed, lens, foff, rowoff, ws, total;
};
__host__ __device__ inline FmtLds fmt_lds(int TR, int m, int slot) {
    auto up16 = [](int v) { return (v + 15) & ~15; };
    FmtLds l;
    l.slots = 0;
    l.packed = up16(TR * m * slot);
    l.lens = l.packed + up16(TR * m * slot + 16);
    l.foff = l.lens + up16(TR * m);
    l.rowoff = l.foff + up16(TR * m * 2);
    l.ws = l.rowoff + up16((TR + 1) * 4);
    l.total = l.ws + FMT_WAVES * GD_FMT_WS_WORDS * 4;
    return l;
}

__device__ __forceinline__ uint64_t fmt_load(const FmtArgs& p, int64_t k, int j) {
    if (!p.srcs) return (uint64_t)__double_as_longlong(p.x[k * p.rs + (int64_t)j * p.cs]);
    const int64_t r = p.rows ? (int64_t)p.rows[k] : p.row_lo + k;
    if (r < 0 || r >= p.N) return 0x7ff8000000000000ULL;
    const int s = p.srcs[j];
    double v;
    if (s >= 0)
        v = p.cols[(int64_t)s * p.ld + r];
    else if (s == GD_FMT_SRC_WEIGHT)
        v = p.w ? p.w[r] : 1.0;
    else
        v = s == GD_FMT_SRC_ONE ? 1.0 : 0.0;
    return (uint64_t)__double_as_longlong(v);
}

// The decimal form of one value per lane; every lane of the wave calls it (`valid` says whether it has a value).
__device__ __forceinline__ void fmt_decimal(uint64_t bits, bool valid, int prec, uint32_t* ws_wave, gdfmt::Decimal* d) {
    const int done = valid ? gdfmt::decimal_fast(bits, prec, d) : 1;
    unsigned long long need = __ballot(!done);
    const int lane = threadIdx.x & 63;
    while (need) {
        const int l = __ffsll((long long)need) - 1;
        need &= need - 1;
        if (lane == l) gdfmt::decimal_slow(bits, prec, ws_wave, d);
    }
}

// bytes of field j with what follows it: one space between fields when sep, '\n' after the last
__device__ __forceinline__ int fmt_tail(const FmtArgs& p, int j) { return j == p.m - 1 ? 1 : p.sep; }

template <bool WRITE>
__global__ void __launch_bounds__(FMT_THREADS) k_format(FmtArgs p, long long* __restrict__ tile_bytes, char* __restrict__ out,
                                                         int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int TR = p.TR, m = p.m;
    const int r = threadIdx.x % TR, j0 = threadIdx.x / TR, jstep = FMT_THREADS / TR;
    const int64_t k = (int64_t)blockIdx.x * TR + r;
    const int rounds = (m + jstep - 1) / jstep;  // the same for every thread: fmt_decimal votes across the wave

    if constexpr (!WRITE) {  // LDS: the wave sums, then the exact path's words (FMT_COUNT_LDS bytes)
        long long* red = (long long*)smem;
        uint32_t* ws_wave = (uint32_t*)(smem + 32) + (threadIdx.x >> 6) * GD_FMT_WS_WORDS;
        long long bytes = 0;
        for (int it = 0; it < rounds; ++it) {
            const int j = j0 + it * jstep;
            const bool valid = j < m && k < p.K;
            gdfmt::Decimal d;
            fmt_decimal(valid ? fmt_load(p, k, j) : 0, valid, p.prec, ws_wave, &d);
            if (valid) bytes += gdfmt::text_length(d, p.width, p.prec) + fmt_tail(p, j);
        }
        bytes = block_sum(bytes, red);
        if (threadIdx.x == 0) tile_bytes[blockIdx.x] = bytes;
        return;
    }

    const FmtLds L = fmt_lds(TR, m, p.slot);
    uint32_t* ws_wave = (uint32_t*)(smem + L.ws) + (threadIdx.x >> 6) * GD_FMT_WS_WORDS;
    char* slots = smem + L.slots;
    char* packed = smem + L.packed;
    unsigned char* lens = (unsigned char*)(smem + L.lens);
    unsigned short* foff = (unsigned short*)(smem + L.foff);
    int* rowoff = (int*)(smem + L.rowoff);

    for (int it = 0; it < rounds; ++it) {
        const int j = j0 + it * jstep;
        const bool valid = j < m && k < p.K;
        gdfmt::Decimal d;
        fmt_decimal(valid ? fmt_load(p, k, j) : 0, valid, p.prec, ws_wave, &d);
        if (valid) {
            char* s = slots + (r * m + j) * p.slot;
            int len = gdfmt::put_text(d, p.width, p.prec, p.upper != 0, s);
            if (j == m - 1)
                s[len++] = '\n';
            else if (p.sep)
                s[len++] = ' ';
            lens[r * m + j] = (unsigned char)len;
        }
    }
    __syncthreads();
    if (threadIdx.x < TR) {  // field offsets inside row r, and the row's length
        int acc = 0;
        if (k < p.K)
            for (int j = 0; j < m; ++j) {
                foff[r * m + j] = (unsigned short)acc;
                acc += lens[r * m + j];
            }
        rowoff[r + 1] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        rowoff[0] = 0;
        for (int i = 0; i < TR; ++i) rowoff[i + 1] += rowoff[i];
    }
    __syncthreads();
    const long long base = tile_bytes[blockIdx.x];  // after the scan: the tile's offset in the text
    char* g = out + base;
    const int phase = (int)((uintptr_t)g & 15);  // packed[phase + i] is byte i of the tile: 16-byte chunks line up
    for (int it = 0; it < rounds; ++it) {
        const int j = j0 + it * jstep;
        if (j < m && k < p.K) {
            const char* s = slots + (r * m + j) * p.slot;
            char* t = packed + phase + rowoff[r] + foff[r * m + j];
            const int len = lens[r * m + j];
            for (int i = 0; i < len; ++i) t[i] = s[i];
        }
    }
    __syncthreads();
    const int end = phase + rowoff[TR];
    for (int lo = threadIdx.x * 16; lo < end; lo += FMT_THREADS * 16) {
        const long long at = base - phase + lo;  // output offset of packed[lo]
        if (lo >= phase && lo + 16 <= end && at + 16 <= capacity) {
            *(uint4*)(out + at) = *(const uint4*)(packed + lo);
        } else {
            const int a = lo < phase ? phase : lo, b = lo + 16 < end ? lo + 16 : end;
            for (int i = a; i < b; ++i)
                if (base - phase + i < capacity) out[base - phase + i] = packed[i];
        }
    }
}

// p holds everything but TR, slot and the device copy of the sources
static int format_common(gd_ctx* ctx, FmtArgs p, const int32_t* srcs_host, void* d_out, int64_t capacity, int64_t* bytes_out) {
    GD_REQUIRE(bytes_out, "null argument");
    GD_REQUIRE(p.m >= 1, "a row has at least one field");
    GD_REQUIRE(p.prec >= 0 && p.prec <= GD_FMT_MAX_PREC, "precision outside 0..17");
    GD_REQUIRE(p.width >= 0 && p.width <= GD_FMT_MAX_WIDTH, "width outside 0..32");
    GD_REQUIRE(capacity >= 0 && (d_out || capacity == 0), "bad text buffer");
    p.slot = (p.width > p.prec + 8 ? p.width : p.prec + 8) + 1;
    GD_REQUIRE((int64_t)p.m * p.slot <= FMT_LDS_BYTES / 2, "too many fields: one row of them does not fit in LDS");
    p.TR = FMT_MAX_TILE_ROWS;
    while (p.TR > 1 && fmt_lds(p.TR, p.m, p.slot).total > FMT_LDS_BYTES) p.TR >>= 1;
    GD_REQUIRE(fmt_lds(p.TR, p.m, p.slot).total <= FMT_LDS_BYTES, "too many fields: one row of them does not fit in LDS");
    *bytes_out = 0;
    if (p.K == 0) return GD_OK;
    const int64_t nb64 = (p.K + p.TR - 1) / p.TR;
    GD_REQUIRE(nb64 < (1LL << 30), "too many rows for one call");
    const int nb = (int)nb64;
    const int64_t cnt_bytes = ((int64_t)nb + 1) * 8;
    char* scr = (char*)gd_scratch(ctx, cnt_bytes + (int64_t)p.m * 4);
    if (!scr) return GD_ERR_NOMEM;
    long long* cnt = (long long*)scr;
    if (srcs_host) {
        GD_TRY(gd_h2d(ctx, scr + cnt_bytes, srcs_host, (size_t)p.m * 4));
        p.srcs = (const int32_t*)(scr + cnt_bytes);
    }
    const size_t lds = (size_t)fmt_lds(p.TR, p.m, p.slot).total;
    k_format<false><<<nb, FMT_THREADS, FMT_COUNT_LDS, ctx->stream>>>(p, cnt, nullptr, 0);
    GD_KERNEL_CHECK();
    long long total = 0;
    GD_TRY(gd_tile_offsets(ctx, cnt, nb, &total));
    GD_TRY(gd_stream_sync(ctx));
    *bytes_out = total;
    if (total > capacity) {
        gd_fail(ctx, GD_FORMAT_MORE_BYTES, "text buffer holds %lld bytes, the text takes %lld", (long long)capacity, total);
        return GD_FORMAT_MORE_BYTES;
    }
    k_format<true><<<nb, FMT_THREADS, lds, ctx->stream>>>(p, cnt, (char*)d_out, capacity);
    GD_KERNEL_CHECK();
    GD_TRY(gd_stream_sync(ctx));
    return GD_OK;
}

extern "C" {

int gd_format_rows(gd_ctx* ctx, const int32_t* srcs, int32_t m, int64_t row_lo, int64_t row_hi, const void* d_rows, int64_t K,
                   int32_t width, int32_t prec, int32_t upper, int32_t sep, void* d_out, int64_t capacity, int64_t* bytes_out) {
    GD_REQUIRE(ctx && srcs && m >= 1, "bad argument");
    GD_REQUIRE(ctx->cols && ctx->N > 0, "no samples uploaded");
    for (int i = 0; i < m; ++i)
        GD_REQUIRE(srcs[i] >= GD_FMT_SRC_ONE && srcs[i] < ctx->n + GD_EXTRA_COLS, "column out of range");
    FmtArgs p = {};
    if (d_rows) {
        GD_REQUIRE(row_lo == 0 && row_hi == 0, "give a row interval or a row list, not both");
        GD_REQUIRE(K >= 0, "bad row count");
        p.rows = (const int32_t*)d_rows;
        p.K = K;
    } else {
        GD_REQUIRE(row_lo >= 0 && row_lo < row_hi && row_hi <= ctx->N, "empty or out-of-range row interval");
        p.row_lo = row_lo;
        p.K = row_hi - row_lo;
    }
    p.cols = ctx->cols, p.ld = ctx->ld, p.N = ctx->N;
    p.w = ctx->w_sel ? ctx->w_main : ctx->w;  // always the sample weights
    p.m = m, p.width = width, p.prec = prec, p.upper = upper, p.sep = sep != 0;
    return format_common(ctx, p, srcs, d_out, capacity, bytes_out);
}

int gd_format_matrix(gd_ctx* ctx, const void* d_x, int64_t K, int32_t m, int64_t row_stride, int64_t col_stride, int32_t width,
                     int32_t prec, int32_t upper, int32_t sep, void* d_out, int64_t capacity, int64_t* bytes_out) {
    GD_REQUIRE(ctx && K >= 0 && m >= 1 && (d_x || K == 0), "bad argument");
    FmtArgs p = {};
    p.x = (const double*)d_x, p.rs = row_stride, p.cs = col_stride, p.K = K;
    p.m = m, p.width = width, p.prec = prec, p.upper = upper, p.sep = sep != 0;
    return format_common(ctx, p, nullptr, d_out, capacity, bytes_out);
}

}  // extern "C"
