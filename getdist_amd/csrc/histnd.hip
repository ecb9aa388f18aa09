// Raw N-D histograms of getRawNDDensityGridData (mcsamples.py:2121-2235): B densities over d_b parameters each, nb bins per
// axis, flat bin q = ix_0 + nb ix_1 + nb^2 ix_2 + ... (the reference's _flattenValues: the first parameter varies fastest).
//
// Indices: every distinct (column, binmin, width) is pre-binned ONCE per call by the existing bit-exact index kernels
// (gd_prebin8_batch: bytes for nb <= 256; gd_prebin_batch: u16 with the 0xFFFF sentinel above) and every density that uses
// it reads that column -- the lever of the triangle.  No new division.
//
// Sums are integers, so any order of the atomics gives the same bits:
//   * unit weights and integral multiplicities (ctx->w_integral: sum < 2^32) add counts;
//   * real weights add round(w 2^k) in 64-bit fixed point with 2^k N max(w) < 2^61 (k from a device max of the vector),
//     and the finish divides by 2^k (exact);
//   * Lmin is the min of an order-preserving u64 encoding of the loglike (integer min), decoded by the finish.
// Two tiers per density:
//   LDS     the block's counters (4 or 8 bytes per output per bin) fit HND_LDS_BYTES: a block privatises the grid of one
//           density for one chunk of rows in LDS (ds_add_u32 / ds_add_u64 / ds_min_u64) and flushes the non-empty bins
//           to the zeroed device grid with global integer atomics;
//   global  larger grids: every sample goes straight to the device grid with global integer atomics.
// Blocks are ordered chunk-major (all densities of one row chunk are neighbours in the grid), so the densities that share
// an index column read the same rows of it at about the same time.
#include "ctx.hpp"

#include <cmath>
#include <map>
#include <tuple>
#include <type_traits>

#define HND_LDS_BYTES (128 * 1024)
#define HND_THREADS 512
#define HND_EMPTY 0xFFFFFFFFFFFFFFFFull  // Lmin of an empty bin (memset 0xFF); decoded to +inf

struct HistNDDesc {
    const void* idx[GD_HISTND_MAXD];  // index columns (u8 or u16), axis 0 first
    int d, M;
    int64_t off;                      // this density's grids start at element `off` of each output
};

__device__ __forceinline__ unsigned long long hnd_enc(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double hnd_dec(unsigned long long e) {
    if (e == HND_EMPTY) return __longlong_as_double(0x7FF0000000000000ll);  // +inf
    return __longlong_as_double((long long)((e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e));
}
// fixed-point scale 2^k with 2^k N max(w) < 2^61 (1 when every weight is 0)
__device__ __forceinline__ double hnd_scale(unsigned long long wmax_bits, int64_t N) {
    const double m = __longlong_as_double((long long)wmax_bits);
    if (!(m > 0)) return 1.0;
    return ldexp(1.0, 60 - ilogb(m * (double)N));
}

// max of a non-negative weight vector: the bits of a non-negative double order like the double.  grid (blocks, 2)
__global__ void __launch_bounds__(256) k_hnd_wmax(const double* __restrict__ w0, const double* __restrict__ w1, int64_t N,
                                                  unsigned long long* __restrict__ out) {
    const double* w = blockIdx.y ? w1 : w0;
    if (!w) return;
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const double v = w[i];
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        if (v > 0 && b > m) m = b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_down(m, o, WAVE);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&out[blockIdx.y], m);
}

// four consecutive index values of one column at row i (i % 4 == 0; the buffers are padded past N)
template <typename IdxT>
__device__ __forceinline__ void hnd_load4(const void* col, int64_t i, unsigned v[4]);
template <>
__device__ __forceinline__ void hnd_load4<unsigned char>(const void* col, int64_t i, unsigned v[4]) {
    const unsigned p = *(const __attribute__((address_space(1))) unsigned*)((const unsigned char*)col + i);
    v[0] = p & 0xffu, v[1] = (p >> 8) & 0xffu, v[2] = (p >> 16) & 0xffu, v[3] = p >> 24;
}
template <>
__device__ __forceinline__ void hnd_load4<unsigned short>(const void* col, int64_t i, unsigned v[4]) {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 p = *(const __attribute__((address_space(1))) u32x2*)((const unsigned short*)col + i);
    v[0] = p.x & 0xffffu, v[1] = p.x >> 16, v[2] = p.y & 0xffffu, v[3] = p.y >> 16;
}

// WM: 0 unit weights, 1 integral multiplicities (u32 counters), 2 real weights (64-bit fixed point).
// grid: nchunks x nlist blocks, chunk-major; list[k] = the density of the k-th block of a chunk.
template <typename IdxT, int WM, bool LDS>
__global__ void __launch_bounds__(HND_THREADS) k_histnd(const HistNDDesc* __restrict__ descs, const int* __restrict__ list,
                                                        int nlist, int64_t N, int64_t rows, int nb, int flags,
                                                        const double* __restrict__ w, const double* __restrict__ lw,
                                                        const double* __restrict__ ll,
                                                        const unsigned long long* __restrict__ wmax,
                                                        unsigned long long* __restrict__ gH, unsigned long long* __restrict__ gHL,
                                                        unsigned long long* __restrict__ gL, unsigned long long* __restrict__ bad) {
    extern __shared__ unsigned long long hnd_sh[];
    const int k = blockIdx.x % nlist;
    const int64_t chunk = blockIdx.x / nlist;
    const HistNDDesc* D = descs + list[k];  // read in place: idx[a] is indexed at run time
    const int M = D->M, d = D->d;
    const bool doH = flags & GD_HISTND_H, doHL = flags & GD_HISTND_LIKES, doL = flags & GD_HISTND_LMIN;
    typedef typename std::conditional<WM == 2, unsigned long long, unsigned int>::type CntT;
    // LDS layout: [H: M CntT][pad to 8][HL: M u64][Lmin: M u64] (only the requested outputs)
    CntT* sH = (CntT*)hnd_sh;
    unsigned long long* sHL = hnd_sh + (doH ? ((int64_t)M * sizeof(CntT) + 7) / 8 : 0);
    unsigned long long* sL = sHL + (doHL ? M : 0);
    unsigned long long* H = gH + D->off;
    unsigned long long* HL = gHL + D->off;
    unsigned long long* L = gL + D->off;
    if (LDS) {
        for (int m = threadIdx.x; m < M; m += HND_THREADS) {
            if (doH) sH[m] = 0;
            if (doHL) sHL[m] = 0;
            if (doL) sL[m] = HND_EMPTY;
        }
        __syncthreads();
    }
    const double sw = (WM == 2 && doH) ? hnd_scale(wmax[0], N) : 1.0;
    const double slw = doHL ? hnd_scale(wmax[1], N) : 1.0;
    const int64_t r0 = chunk * rows, r1 = r0 + rows < N ? r0 + rows : N;
    unsigned nbad = 0;
    for (int64_t i = r0 + 4 * (int64_t)threadIdx.x; i < r1; i += 4 * HND_THREADS) {
        unsigned q[4] = {0, 0, 0, 0};
        bool ok[4] = {true, true, true, true};
        unsigned stride = 1;
        for (int a = 0; a < d; ++a) {
            unsigned v[4];
            hnd_load4<IdxT>(D->idx[a], i, v);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ok[r] = ok[r] && v[r] < (unsigned)nb;
                q[r] += v[r] * stride;
            }
            stride *= (unsigned)nb;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = i + r;
            if (row >= r1) break;
            if (!ok[r] || q[r] >= (unsigned)M) {
                ++nbad;
                continue;
            }
            if (doH) {
                if (WM == 0) {
                    if (LDS) atomicAdd((unsigned int*)&sH[q[r]], 1u);
                    else atomicAdd(&H[q[r]], 1ull);
                } else if (WM == 1) {
                    const unsigned c = (unsigned)w[row];
                    if (c) {
                        if (LDS) atomicAdd((unsigned int*)&sH[q[r]], c);
                        else atomicAdd(&H[q[r]], (unsigned long long)c);
                    }
                } else {
                    const unsigned long long c = __double2ull_rn(w[row] * sw);
                    if (c) {
                        if (LDS) atomicAdd((unsigned long long*)&sH[q[r]], c);
                        else atomicAdd(&H[q[r]], c);
                    }
                }
            }
            if (doHL) {
                const unsigned long long c = __double2ull_rn(lw[row] * slw);
                if (c) {
                    if (LDS) atomicAdd(&sHL[q[r]], c);
                    else atomicAdd(&HL[q[r]], c);
                }
            }
            if (doL) {
                const unsigned long long e = hnd_enc(ll[row]);
                if (LDS) atomicMin(&sL[q[r]], e);
                else atomicMin(&L[q[r]], e);
            }
        }
    }
    if (nbad) atomicAdd(bad, (unsigned long long)nbad);
    if (LDS) {
        __syncthreads();
        for (int m = threadIdx.x; m < M; m += HND_THREADS) {
            if (doH && sH[m]) atomicAdd(&H[m], (unsigned long long)sH[m]);
            if (doHL && sHL[m]) atomicAdd(&HL[m], sHL[m]);
            if (doL && sL[m] != HND_EMPTY) atomicMin(&L[m], sL[m]);
        }
    }
}

// integer grids -> fp64 in place: counts as they are, fixed point / 2^k, Lmin decoded
__global__ void __launch_bounds__(256) k_histnd_finish(unsigned long long* __restrict__ H, unsigned long long* __restrict__ HL,
                                                       unsigned long long* __restrict__ L, int64_t total, int flags, int real_w,
                                                       const unsigned long long* __restrict__ wmax, int64_t N) {
    const double sw = real_w ? hnd_scale(wmax[0], N) : 1.0, slw = hnd_scale(wmax[1], N);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        if (flags & GD_HISTND_H) {
            const double v = (double)H[i] / sw;
            H[i] = (unsigned long long)__double_as_longlong(v);
        }
        if (flags & GD_HISTND_LIKES) {
            const double v = (double)HL[i] / slw;
            HL[i] = (unsigned long long)__double_as_longlong(v);
        }
        if (flags & GD_HISTND_LMIN) L[i] = (unsigned long long)__double_as_longlong(hnd_dec(L[i]));
    }
}

template <typename IdxT, int WM>
static int launch_histnd(gd_ctx* ctx, bool lds, const HistNDDesc* d_desc, const int* d_list, int nlist, int nchunks,
                         int64_t rows, int nb, int flags, const double* lw, const double* ll, size_t lds_bytes,
                         const unsigned long long* d_wmax, unsigned long long* gH, unsigned long long* gHL,
                         unsigned long long* gL, unsigned long long* d_bad) {
    const dim3 grid((unsigned)((int64_t)nchunks * nlist));
    if (lds) {
        GD_HIP(hipFuncSetAttribute((const void*)k_histnd<IdxT, WM, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   HND_LDS_BYTES));
        k_histnd<IdxT, WM, true><<<grid, HND_THREADS, lds_bytes, ctx->stream>>>(
            d_desc, d_list, nlist, ctx->N, rows, nb, flags, ctx->w, lw, ll, d_wmax, gH, gHL, gL, d_bad);
    } else {
        k_histnd<IdxT, WM, false><<<grid, HND_THREADS, 0, ctx->stream>>>(
            d_desc, d_list, nlist, ctx->N, rows, nb, flags, ctx->w, lw, ll, d_wmax, gH, gHL, gL, d_bad);
    }
    GD_KERNEL_CHECK();
    return GD_OK;
}

template <typename IdxT>
static int launch_histnd_w(gd_ctx* ctx, int wm, bool lds, const HistNDDesc* d_desc, const int* d_list, int nlist,
                           int nchunks, int64_t rows, int nb, int flags, const double* lw, const double* ll, size_t lds_bytes,
                           const unsigned long long* d_wmax, unsigned long long* gH, unsigned long long* gHL,
                           unsigned long long* gL, unsigned long long* d_bad) {
    if (wm == 0)
        return launch_histnd<IdxT, 0>(ctx, lds, d_desc, d_list, nlist, nchunks, rows, nb, flags, lw, ll, lds_bytes, d_wmax,
                                      gH, gHL, gL, d_bad);
    if (wm == 1)
        return launch_histnd<IdxT, 1>(ctx, lds, d_desc, d_list, nlist, nchunks, rows, nb, flags, lw, ll, lds_bytes, d_wmax,
                                      gH, gHL, gL, d_bad);
    return launch_histnd<IdxT, 2>(ctx, lds, d_desc, d_list, nlist, nchunks, rows, nb, flags, lw, ll, lds_bytes, d_wmax, gH,
                                  gHL, gL, d_bad);
}

// row chunks per density: enough blocks to fill the device, chunks of at least 64 K rows (a multiple of 4)
static void hnd_chunks(const gd_ctx* ctx, int nlist, int per_cu, int& nchunks, int64_t& rows) {
    const int64_t N = ctx->N;
    int64_t want = ((int64_t)per_cu * ctx->cu_count + nlist - 1) / nlist;
    const int64_t most = (N + 65535) / 65536;
    if (want > most) want = most;
    if (want < 1) want = 1;
    rows = (N + want - 1) / want;
    rows = (rows + 3) / 4 * 4;
    nchunks = (int)((N + rows - 1) / rows);
    if (nchunks < 1) nchunks = 1;
}

extern "C" {

int gd_histnd_batch(gd_ctx* ctx, int32_t B, const int32_t* dims, const int32_t* cols, const double* binmin,
                    const double* width, int32_t nb, int32_t flags, int32_t loglike_col, double* H_out, double* HL_out,
                    double* Lmin_out) {
    GD_REQUIRE(ctx && dims && cols && binmin && width && B > 0, "bad argument");
    GD_REQUIRE(ctx->cols, "no samples uploaded");
    GD_REQUIRE(nb >= 2 && nb < 65535, "num_bins_ND out of range (2..65534)");
    GD_REQUIRE(flags > 0 && (flags & ~(GD_HISTND_H | GD_HISTND_LIKES | GD_HISTND_LMIN)) == 0, "bad output flags");
    GD_REQUIRE(!(flags & GD_HISTND_H) || H_out, "H_out is null");
    GD_REQUIRE(!(flags & GD_HISTND_LIKES) || HL_out, "HL_out is null");
    GD_REQUIRE(!(flags & GD_HISTND_LMIN) || Lmin_out, "Lmin_out is null");
    GD_REQUIRE(!(flags & GD_HISTND_LIKES) || ctx->like_w, "no like weights: call gd_like_weights (mode 0) first");
    GD_REQUIRE(!(flags & GD_HISTND_LMIN) || (loglike_col >= 0 && loglike_col < ctx->n + GD_EXTRA_COLS),
               "loglike column out of range");
    GD_REQUIRE(ctx->N > 0 && ctx->N < ((int64_t)1 << 31), "sample count out of range for the N-D counters");
    const int64_t N = ctx->N;
    // per density: shape, grid offset; distinct (column, binmin, width) index columns
    std::vector<HistNDDesc> hd((size_t)B);
    std::vector<int> first((size_t)B + 1, 0);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        GD_REQUIRE(dims[b] >= 1 && dims[b] <= GD_HISTND_MAXD, "dimension out of range (1..GD_HISTND_MAXD)");
        int64_t M = 1;
        for (int a = 0; a < dims[b]; ++a) {
            M *= nb;
            GD_REQUIRE(M <= GD_HISTND_MAX_BINS, "grid larger than GD_HISTND_MAX_BINS bins");
        }
        first[b + 1] = first[b] + dims[b];
        memset(&hd[b], 0, sizeof(HistNDDesc));
        hd[b].d = dims[b], hd[b].M = (int)M, hd[b].off = total;
        total += M;
    }
    std::map<std::tuple<int, double, double>, int> uniq;
    std::vector<int32_t> ucol;
    std::vector<double> ubmin, uwidth;
    std::vector<int> slot((size_t)first[B]);
    GD_REQUIRE_COLUMNS(cols, first[B]);
    for (int t = 0; t < first[B]; ++t) {
        GD_REQUIRE(cols[t] >= 0 && cols[t] < ctx->n + GD_EXTRA_COLS, "column out of range");
        GD_REQUIRE(width[t] > 0 && std::isfinite(width[t]) && std::isfinite(binmin[t]), "bad bin width / origin");
        const auto key = std::make_tuple((int)cols[t], binmin[t], width[t]);
        auto it = uniq.find(key);
        if (it == uniq.end()) {
            it = uniq.emplace(key, (int)ucol.size()).first;
            ucol.push_back(cols[t]), ubmin.push_back(binmin[t]), uwidth.push_back(width[t]);
        }
        slot[t] = it->second;
    }
    const int nu = (int)ucol.size();
    const bool u8 = nb <= 256;
    // tiers
    const int wm = !ctx->w ? 0 : (ctx->w_integral ? 1 : 2);
    const int hbytes = (flags & GD_HISTND_H) ? (wm == 2 ? 8 : 4) : 0;
    const int bpb = hbytes + ((flags & GD_HISTND_LIKES) ? 8 : 0) + ((flags & GD_HISTND_LMIN) ? 8 : 0);
    std::vector<int> lds_list, glob_list;
    int Mmax_lds = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t need = ((int64_t)hd[b].M * hbytes + 7) / 8 * 8 + (int64_t)hd[b].M * (bpb - hbytes);
        if (need <= HND_LDS_BYTES && !getenv("GDHIP_HISTND_GLOBAL")) {
            lds_list.push_back(b);
            if (hd[b].M > Mmax_lds) Mmax_lds = hd[b].M;
        } else {
            glob_list.push_back(b);
        }
    }
    // device scratch: index columns, descriptors, lists, grids (u64 per output), max words, bad counter
    ScratchPlan sp;
    std::vector<ScratchPlan::Buf<unsigned char>> d_idx;  // padded by 64 rows: the kernel reads 4 rows at a time
    for (int u = 0; u < nu; ++u) d_idx.push_back(sp.take<unsigned char>((N + 64) * (u8 ? 1 : 2)));
    auto d_desc = sp.take<HistNDDesc>(B);
    auto d_list = sp.take<int>(B);
    auto gH = sp.take<unsigned long long>((flags & GD_HISTND_H) ? total : 1);
    auto gHL = sp.take<unsigned long long>((flags & GD_HISTND_LIKES) ? total : 1);
    auto gL = sp.take<unsigned long long>((flags & GD_HISTND_LMIN) ? total : 1);
    auto d_wmax = sp.take<unsigned long long>(8);  // two maxima, then the bad-sample counter
    GD_TRY(sp.get(ctx));
    std::vector<void*> ubuf(d_idx.begin(), d_idx.end());
    for (int b = 0; b < B; ++b)
        for (int a = 0; a < dims[b]; ++a) hd[b].idx[a] = ubuf[slot[first[b] + a]];
    // index columns (these calls wait for their kernels: the columns are complete when they return)
    if (u8) {
        std::vector<int64_t> nbad((size_t)nu, 0);
        GD_TRY(gd_prebin8_batch(ctx, ucol.data(), nu, ubmin.data(), uwidth.data(), nb, ubuf.data(), nbad.data()));
        for (int u = 0; u < nu; ++u)
            if (nbad[u]) return gd_fail(ctx, GD_ERR_BADARG, "%lld samples of column %d fall outside the %d bins",
                                        (long long)nbad[u], (int)ucol[u], (int)nb);
    } else {
        GD_TRY(gd_prebin_batch(ctx, ucol.data(), nu, ubmin.data(), uwidth.data(), nb, ubuf.data()));
    }
    unsigned long long* d_bad = d_wmax + 2;
    std::vector<int> lists(lds_list);
    lists.insert(lists.end(), glob_list.begin(), glob_list.end());
    GD_TRY(gd_h2d(ctx, d_desc, hd.data(), (size_t)B * sizeof(HistNDDesc)));
    GD_TRY(gd_h2d(ctx, d_list, lists.data(), (size_t)B * 4));
    GD_HIP(hipMemsetAsync(d_wmax, 0, 64, ctx->stream));
    if (flags & GD_HISTND_H) GD_HIP(hipMemsetAsync(gH, 0, (size_t)total * 8, ctx->stream));
    if (flags & GD_HISTND_LIKES) GD_HIP(hipMemsetAsync(gHL, 0, (size_t)total * 8, ctx->stream));
    if (flags & GD_HISTND_LMIN) GD_HIP(hipMemsetAsync(gL, 0xFF, (size_t)total * 8, ctx->stream));
    const double* lw = (flags & GD_HISTND_LIKES) ? ctx->like_w : nullptr;
    const double* ll = (flags & GD_HISTND_LMIN) ? ctx->cols + (int64_t)loglike_col * ctx->ld : nullptr;
    const double* wreal = (wm == 2 && (flags & GD_HISTND_H)) ? ctx->w : nullptr;
    if (wreal || lw) {
        k_hnd_wmax<<<dim3(2 * ctx->cu_count, 2), 256, 0, ctx->stream>>>(wreal, lw, N, d_wmax);
        GD_KERNEL_CHECK();
    }
    if (!lds_list.empty()) {
        int nchunks;
        int64_t rows;
        hnd_chunks(ctx, (int)lds_list.size(), 4, nchunks, rows);
        const size_t lds = (size_t)(((int64_t)Mmax_lds * hbytes + 7) / 8 * 8 + (int64_t)Mmax_lds * (bpb - hbytes));
        if (u8)
            GD_TRY(launch_histnd_w<unsigned char>(ctx, wm, true, d_desc, d_list, (int)lds_list.size(), nchunks, rows, nb, flags,
                                                  lw, ll, lds, d_wmax, gH, gHL, gL, d_bad));
        else
            GD_TRY(launch_histnd_w<unsigned short>(ctx, wm, true, d_desc, d_list, (int)lds_list.size(), nchunks, rows, nb, flags,
                                                   lw, ll, lds, d_wmax, gH, gHL, gL, d_bad));
    }
    if (!glob_list.empty()) {
        int nchunks;
        int64_t rows;
        hnd_chunks(ctx, (int)glob_list.size(), 8, nchunks, rows);
        const int* gl = d_list + lds_list.size();
        if (u8)
            GD_TRY(launch_histnd_w<unsigned char>(ctx, wm, false, d_desc, gl, (int)glob_list.size(), nchunks, rows, nb, flags, lw,
                                                  ll, 0, d_wmax, gH, gHL, gL, d_bad));
        else
            GD_TRY(launch_histnd_w<unsigned short>(ctx, wm, false, d_desc, gl, (int)glob_list.size(), nchunks, rows, nb, flags,
                                                   lw, ll, 0, d_wmax, gH, gHL, gL, d_bad));
    }
    {
        int64_t nblk = (total + 255) / 256;
        if (nblk > 4 * ctx->cu_count) nblk = 4 * ctx->cu_count;
        k_histnd_finish<<<(unsigned)nblk, 256, 0, ctx->stream>>>(gH, gHL, gL, total, flags, wm == 2, d_wmax, N);
        GD_KERNEL_CHECK();
    }
    unsigned long long nbad = 0;
    GD_TRY(gd_fetch(ctx, &nbad, d_bad, 8));
    if (flags & GD_HISTND_H) GD_TRY(gd_fetch(ctx, H_out, gH, (size_t)total * 8));
    if (flags & GD_HISTND_LIKES) GD_TRY(gd_fetch(ctx, HL_out, gHL, (size_t)total * 8));
    if (flags & GD_HISTND_LMIN) GD_TRY(gd_fetch(ctx, Lmin_out, gL, (size_t)total * 8));
    GD_TRY(gd_stream_sync(ctx));
    if (nbad) return gd_fail(ctx, GD_ERR_BADARG, "%llu bin indices outside the grid", nbad);
    return GD_OK;
}

}  // extern "C"
