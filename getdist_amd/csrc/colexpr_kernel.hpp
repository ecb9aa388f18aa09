// The kernel and launch code of gd_expr_eval (colexpr.hip) and gd_expr_eval_tab (coltab.hip).
//
// Column expressions (colexpr.ColumnExpr): one fused pass that evaluates a postfix program per sample row over the
// resident columns -- the derived vector  sigma8 * sqrt(omegam / 0.3)  or the mask  (H0 > 70) & (omegam < 0.3)  -- into a
// spare column, the auxiliary weight buffer or a host vector.
//
// The program travels BY VALUE in the kernel arguments (gdex::Program, ~850 bytes): op and argument of every step are
// scalar loads from the kernarg segment, the dispatch on the op is a scalar branch that the whole wave takes together,
// and constants are SGPR operands.  A lane owns two consecutive rows (one 16-byte load per column it reads).  Per round
// of the grid-stride loop a lane
//   1. stages the distinct columns the program reads in LDS, sc[source][thread], four loads in flight at a time -- an
//      interpreter that loaded at each COL step would have ONE load in flight per wave;
//   2. walks the program with the top of the evaluation stack in registers and the rest in LDS, st[depth][thread]: a
//      runtime-indexed private array would live in scratch memory, while [depth][thread] puts the 64 lanes of a wave on
//      consecutive 16-byte words whatever the depth (no bank conflicts).  Every LDS word is private to its thread: no
//      barrier inside the loop;
//   3. stores the two values (one 16-byte store where both rows exist) and folds them into its min / max / non-zero /
//      NaN tallies.
// LDS is sized per launch from the program: (sources + deepest stack - 1) * 4 KiB, 16 KiB for the S8 example (the
// registers, not LDS, then bound the blocks per CU), 124 KiB at both limits.  The grid is the number of blocks resident at
// once, at most EX_MAX_BLOCKS.  Block partials of the tallies are added on the host in block order.
//
// Table look-ups (gd_expr_eval_tab: GD_TAB_INTERP / SPLINE1 / SPLINE2, colexpr.hpp) run in a SECOND instantiation of the
// kernel, k_expr_eval<true>, whose arguments also carry the descriptors of up to GD_TAB_MAX_TABLES tables that the entry
// point copied into the context's scratch ahead of the launch; k_expr_eval<false> is the kernel without them, and a program
// without tables runs the code it always ran.  A look-up bisects the knot array (tab_upper: ceil(log2 n) dependent loads,
// the same count in every lane) and then reads the 2 to 16 values of its interval.  Each block first copies knot arrays
// into LDS behind its evaluation stack, as many as fit without costing a resident block (ex_eval decides); the others are
// searched in global memory.
#pragma once
#include "ctx.hpp"

#include "colexpr.hpp"

#include <cmath>
#include <vector>

#define EX_THREADS 256
#define EX_MAX_BLOCKS 2048
#define EX_MAX_LDS ((GD_EX_MAX_COLS + GD_EX_MAX_STACK - 1) * EX_THREADS * (int)sizeof(gdex::Pair))  // 124 KiB
#define EX_CU_LDS (160 * 1024)  // LDS of a gfx950 CU
#define EX_STATIC_LDS 256       // what the kernel declares statically (32 bytes), with room to spare

struct ExArgs {
    gdex::Program P;
    const double* srcp[GD_EX_MAX_COLS];  // row 0 of source k; nullptr = the unit weights of an unweighted set
    const double* wmul;                  // GD_EX_TO_AUXW: the sample weights the value is multiplied by (nullptr: 1.0)
    double* out_f64;                     // value of row r goes to out_f64[r - base] ...
    unsigned char* out_u8;               // ... or (GD_EX_TO_HOST_U8) its truth to out_u8[r - base]
    double* part;                        // 4 tallies per block, or nullptr
    int64_t base, lo, hi;                // rows [lo, hi); base = lo rounded down to even: pair p is rows base + 2p, + 1
    int mode;
};

__device__ __forceinline__ gdex::Pair ex_load2(const double* p) {
    const double2 v = gload_d2(p);
    return gdex::Pair{v.x, v.y};
}

struct ExArgsTab : ExArgs {
    gd_expr_table tab[GD_TAB_MAX_TABLES];  // p0 / p1 / p2 are device pointers here
    int32_t stage[GD_TAB_MAX_TABLES][2];   // where the block keeps the knots p0 / (SPLINE2) p1 in LDS: an offset in doubles behind
                                           // the evaluation stack, or -1 for knots that are searched where they are
    int32_t ntab;
};
template <bool TAB>
struct ExKernArgs {
    typedef ExArgs type;
};
template <>
struct ExKernArgs<true> {
    typedef ExArgsTab type;
};

// TAB: the program may hold table ops, and the arguments carry their tables (k_expr_eval<false> is the kernel of a program
// without: no table code, no table arguments)
// grid: min(resident blocks, EX_MAX_BLOCKS, ceil(pairs / 256)) blocks of 256; dynamic LDS: sc[nsrc][256] | st[depth - 1][256] of Pair
template <bool TAB>
__global__ void __launch_bounds__(EX_THREADS) k_expr_eval(typename ExKernArgs<TAB>::type A) {
    extern __shared__ double2 ex_lds[];
    __shared__ double red[EX_THREADS / 64];
    gdex::Pair* sc = (gdex::Pair*)ex_lds;
    const int tid = threadIdx.x;
    const int nsrc = A.P.nsrc, ncode = A.P.ncode;
    gdex::Pair* st = sc + nsrc * EX_THREADS;
    const int64_t npairs = (A.hi - A.base + 1) >> 1;
    double mn = INFINITY, mx = -INFINITY, nz = 0.0, nn = 0.0;
    double* lk = nullptr;  // the knots staged in LDS, once per block
    if constexpr (TAB) {
        lk = (double*)(st + (A.P.depth - 1) * EX_THREADS);
        for (int k = 0; k < A.ntab; ++k)
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const int off = A.stage[k][part];
                if (off < 0) continue;
                const double* src = part ? A.tab[k].p1 : A.tab[k].p0;
                const int n = part ? A.tab[k].ny : A.tab[k].nx;
                for (int i = tid; i < n; i += EX_THREADS) lk[off + i] = src[i];
            }
        __syncthreads();
    }
    for (int64_t p = (int64_t)blockIdx.x * EX_THREADS + tid; p < npairs; p += (int64_t)gridDim.x * EX_THREADS) {
        // both rows lie inside the columns' leading dimension (even, >= N): loads need no guard, stores do
        const int64_t r = A.base + 2 * p;
        gdex::Pair wv{1.0, 1.0};
        if (A.mode == GD_EX_TO_AUXW && A.wmul) wv = ex_load2(A.wmul + r);
        for (int c0 = 0; c0 < nsrc; c0 += 4) {
            gdex::Pair v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < nsrc) {
                    const double* s = A.srcp[c0 + k];
                    v[k] = s ? ex_load2(s + r) : gdex::Pair{1.0, 1.0};
                }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < nsrc) sc[(c0 + k) * EX_THREADS + tid] = v[k];
        }
        gdex::Pair top{0.0, 0.0};
        int d = 0;  // entries on the stack: 0 .. d - 2 in st, d - 1 in `top`
        for (int pc = 0; pc < ncode; ++pc) {
            const unsigned ins = A.P.ins[pc];  // a scalar load: the address is wave-uniform
            const int op = (int)(ins & 0xffu), a = (int)(ins >> 8);
            if (op <= GD_EX_CONST) {
                if (d > 0) st[(d - 1) * EX_THREADS + tid] = top;
                if (op == GD_EX_COL) {
                    top = sc[a * EX_THREADS + tid];
                } else {
                    const double c = A.P.consts[a];
                    top = gdex::Pair{c, c};
                }
                ++d;
            } else if (op <= GD_EX_NOT) {
                top = gdex::ex_apply1(op, top);
            } else if (op <= GD_EX_OR) {
                top = gdex::ex_apply2(op, st[(d - 2) * EX_THREADS + tid], top);
                --d;
            } else if (!TAB || op == GD_EX_WHERE) {
                top = gdex::map_where(st[(d - 3) * EX_THREADS + tid], st[(d - 2) * EX_THREADS + tid], top);
                d -= 2;
            } else if constexpr (TAB) {
                const gd_expr_table& T = A.tab[a];  // wave-uniform: the descriptor comes by scalar loads
                const int s0 = A.stage[a][0], s1 = A.stage[a][1];
                const double *k0 = s0 >= 0 ? lk + s0 : T.p0, *k1 = s1 >= 0 ? lk + s1 : T.p1;
                gdex::Pair below{0.0, 0.0};
                if (op == GD_TAB_SPLINE2) below = st[(d - 2) * EX_THREADS + tid], --d;
                top = gdex::Pair{gdex::tab_apply(op, T, k0, k1, below.x, top.x), gdex::tab_apply(op, T, k0, k1, below.y, top.y)};
            }
        }
        const bool ok0 = r >= A.lo, ok1 = r + 1 < A.hi;  // (r < hi and r + 1 >= lo hold for every pair)
        if (A.part) {
            if (ok0) {
                if (top.x != top.x) nn += 1.0; else mn = fmin(mn, top.x), mx = fmax(mx, top.x);
                if (top.x != 0.0) nz += 1.0;
            }
            if (ok1) {
                if (top.y != top.y) nn += 1.0; else mn = fmin(mn, top.y), mx = fmax(mx, top.y);
                if (top.y != 0.0) nz += 1.0;
            }
        }
        if (A.mode == GD_EX_TO_HOST_U8) {
            unsigned char* o = A.out_u8 + (r - A.base);
            if (ok0) o[0] = top.x != 0.0 ? 1 : 0;
            if (ok1) o[1] = top.y != 0.0 ? 1 : 0;
        } else {
            if (A.mode == GD_EX_TO_AUXW) top.x = wv.x * top.x, top.y = wv.y * top.y;
            double* o = A.out_f64 + (r - A.base);
            if (ok0 && ok1)
                *(double2*)o = make_double2(top.x, top.y);
            else if (ok0)
                o[0] = top.x;
            else if (ok1)
                o[1] = top.y;
        }
    }
    if (A.part) {
        mn = block_min(mn, red);
        mx = block_max(mx, red);
        nz = block_sum(nz, red);
        nn = block_sum(nn, red);
        if (tid == 0) {
            double* q = A.part + (int64_t)blockIdx.x * 4;
            q[0] = mn, q[1] = mx, q[2] = nz, q[3] = nn;
        }
    }
}

// The entry points' common part.  TAB = false: gd_expr_eval (tables = nullptr, ntab = 0); TAB = true: gd_expr_eval_tab with
// ntab >= 1.  Each is instantiated in a translation unit of its own (colexpr.hip, coltab.hip), so that the kernel of
// table-free programs is compiled exactly as it was before there were tables: in one unit the two kernels would share their
// callees, and the inliner would treat those otherwise.
template <bool TAB>
static int ex_eval(gd_ctx* ctx, const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int32_t dst,
                   int32_t dst_arg, int64_t lo, int64_t hi, void* host_out, double* stats_out, const gd_expr_table* tables,
                   int32_t ntab) {
    GD_REQUIRE(ctx && code, "null argument");
    GD_REQUIRE(ctx->cols && ctx->N > 0, "no samples uploaded");
    GD_REQUIRE(dst >= GD_EX_TO_COLUMN && dst <= GD_EX_TO_HOST_U8, "unknown destination");
    GD_REQUIRE_ROWS(lo, hi);
    const bool to_host = dst == GD_EX_TO_HOST_F64 || dst == GD_EX_TO_HOST_U8;
    if (to_host) {
        GD_REQUIRE(host_out, "null argument");
    } else {
        GD_REQUIRE(lo == 0 && hi == ctx->N, "a device destination covers every row: lo = 0, hi = N");
    }
    if (dst == GD_EX_TO_COLUMN) GD_REQUIRE(dst_arg >= 0 && dst_arg < GD_EXTRA_COLS, "extra column slot out of range");
    if (dst == GD_EX_TO_AUXW)
        GD_REQUIRE(ctx->w_sel == 0, "auxiliary weights are selected; call gd_select_weights(ctx, 0) first");
    typename ExKernArgs<TAB>::type A{};
    const char* bad = gdex::ex_pack(code, ncode, consts, nconst, ctx->n + GD_EXTRA_COLS, &A.P, tables, ntab);
    if (bad) return gd_fail(ctx, GD_ERR_BADARG, "%s", bad);
    const void* kern = (const void*)k_expr_eval<TAB>;

    const double* sw = ctx->w_sel ? ctx->w_main : ctx->w;  // always the sample weights
    for (int k = 0; k < A.P.nsrc; ++k)
        A.srcp[k] = A.P.src[k] == GD_EX_WEIGHT ? sw : ctx->cols + (int64_t)A.P.src[k] * ctx->ld;
    A.base = lo & ~(int64_t)1, A.lo = lo, A.hi = hi, A.mode = dst;
    const int64_t npairs = (hi - A.base + 1) >> 1;
    size_t lds = (size_t)(A.P.nsrc + A.P.depth - 1) * EX_THREADS * sizeof(gdex::Pair);
    // the attribute belongs to the function, not to the call: always the largest size a valid program can ask for, so that
    // a thread with another context can never lower it between this thread's set and its launch
    GD_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, TAB ? EX_CU_LDS - EX_STATIC_LDS : EX_MAX_LDS));
    if constexpr (TAB) {
        // Knot arrays are staged in LDS, in table order, as long as that costs no resident block: the runtime says how many
        // blocks per CU the registers and the program's own LDS (which may be none: a look-up on a constant) admit, and the
        // staging gets what is left of one block's share of the CU's LDS.  -DGD_TAB_NO_STAGING builds a library that never
        // stages (every search in global memory), for the comparison scripts/bench_coltab.py records.
        int blocks = 0;
        GD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kern, EX_THREADS, lds));
        if (blocks < 1) blocks = 1;
        int64_t avail = EX_CU_LDS / blocks - EX_STATIC_LDS - (int64_t)lds;
#ifdef GD_TAB_NO_STAGING
        avail = 0;
#endif
        int32_t off = 0;
        A.ntab = ntab;
        for (int k = 0; k < ntab; ++k)
            for (int part = 0; part < 2; ++part) {
                const int64_t n = part == 0 ? tables[k].nx : (tables[k].kind == GD_TAB_SPLINE2 ? tables[k].ny : 0);
                A.stage[k][part] = -1;
                if (n > 0 && n * 8 <= avail) A.stage[k][part] = off, off += (int32_t)n, avail -= n * 8;
            }
        lds += (size_t)off * 8;
    }
    // no more blocks than are resident at once (the grid-stride loop takes the rest): blocks beyond that would run as a
    // second, partly filled wave of blocks
    int per_cu = 0;
    GD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, EX_THREADS, lds));
    int64_t cap = (int64_t)(per_cu > 0 ? per_cu : 1) * ctx->cu_count;
    if (cap > EX_MAX_BLOCKS) cap = EX_MAX_BLOCKS;
    int64_t nblk = (npairs + EX_THREADS - 1) / EX_THREADS;
    if (nblk > cap) nblk = cap;

    // scratch: block partials | staging of a host destination (index 0 = row `base`) | the tables
    int64_t tab_doubles = 0;
    for (int k = 0; k < ntab; ++k)
        for (int part = 0; part < 3; ++part) tab_doubles += gdex::tab_doubles(tables[k], part);
    ScratchPlan sp;
    auto d_part = sp.take<double>(nblk * 4);
    auto d_stage = sp.take<unsigned char>(to_host ? 2 * npairs * (dst == GD_EX_TO_HOST_F64 ? 8 : 1) : 0);
    auto d_tabs = sp.tail<double>(tab_doubles);
    GD_TRY(sp.get(ctx));
    if constexpr (TAB) {
        double* d_tab = d_tabs;
        for (int k = 0; k < ntab; ++k) {
            A.tab[k] = tables[k];
            const double* src[3] = {tables[k].p0, tables[k].p1, tables[k].p2};
            const double* at[3] = {nullptr, nullptr, nullptr};
            for (int part = 0; part < 3; ++part) {
                const int64_t nd = gdex::tab_doubles(tables[k], part);
                if (!nd) continue;
                GD_HIP(hipMemcpyAsync(d_tab, src[part], (size_t)nd * 8, hipMemcpyHostToDevice, ctx->stream));
                at[part] = d_tab, d_tab += nd;
            }
            A.tab[k].p0 = at[0], A.tab[k].p1 = at[1], A.tab[k].p2 = at[2];
        }
    }
    A.part = stats_out ? d_part.ptr() : nullptr;
    if (dst == GD_EX_TO_COLUMN) {
        A.out_f64 = ctx->cols + (ctx->n + dst_arg) * ctx->ld;
    } else if (dst == GD_EX_TO_AUXW) {
        if (!ctx->like_w) {
            GD_HIP(hipMalloc((void**)&ctx->like_w, (size_t)(ctx->ld * 8)));
            GD_HIP(hipMemsetAsync(ctx->like_w, 0, (size_t)(ctx->ld * 8), ctx->stream));
        }
        A.out_f64 = ctx->like_w;
        A.wmul = sw;
    } else if (dst == GD_EX_TO_HOST_F64) {
        A.out_f64 = (double*)d_stage.ptr();
    } else {
        A.out_u8 = d_stage;
    }
    k_expr_eval<TAB><<<dim3((unsigned)nblk), EX_THREADS, lds, ctx->stream>>>(A);
    GD_KERNEL_CHECK();
    std::vector<double> part;
    if (stats_out) {
        part.resize((size_t)nblk * 4);
        GD_TRY(gd_fetch(ctx, part.data(), A.part, part.size() * 8));
    }
    if (dst == GD_EX_TO_HOST_F64)
        GD_TRY(gd_memcpy_d2h_async(ctx, host_out, A.out_f64 + (lo - A.base), (hi - lo) * 8));
    else if (dst == GD_EX_TO_HOST_U8)
        GD_TRY(gd_memcpy_d2h_async(ctx, host_out, A.out_u8 + (lo - A.base), hi - lo));
    GD_TRY(gd_stream_sync(ctx));
    if (to_host) GD_TRY(gd_copy_sync(ctx));
    if (stats_out) {
        double mn = INFINITY, mx = -INFINITY, nz = 0, nn = 0;
        for (int64_t b = 0; b < nblk; ++b) {
            mn = std::fmin(mn, part[4 * b]), mx = std::fmax(mx, part[4 * b + 1]);
            nz += part[4 * b + 2], nn += part[4 * b + 3];
        }
        if (nn > 0) mn = mx = NAN;
        stats_out[0] = mn, stats_out[1] = mx, stats_out[2] = nz, stats_out[3] = nn;
    }
    return GD_OK;
}
