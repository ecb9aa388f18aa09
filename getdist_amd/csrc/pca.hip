// Principal components of parameters (MCSamples.PCA, mcsamples.py:682-885): the O(N) passes on the device.
//
// Every pass is a weighted product of two sets of VIRTUAL columns that exist only in registers and LDS:
//   corr mode  (gd_pca_corr)     v_c = map_c(x_c) - centre_c                      (map: N = x, L = log x, M = log -x)
//   proj mode  (gd_pca_project)  p_c = f(sum_k U[c][k] z_k) - centre_c,  z_k = (map_k(x_k) - mean_k) / sd'_k,
//                                f = exp when doexp, else the identity; right-hand columns also
//                                (x_j - all_mean_j) / all_sd_j over the first n_all resident columns
// A block walks a chunk of rows in slabs of KS rows; per slab it stages the slab's weights, (proj) all np z values of every
// row, and the 16-column tiles of its left / right range, then accumulates 16 x 16 tile products
//   S[i][j] += sum_rows (w v_i) v_j       with v_mfma_f64_16x16x4_f64,
// the accumulators staying in registers for the whole chunk.  A pass whose right side is "ones" (B column 0 = 1) delivers
// the weighted column sums, and a left column of ones beyond the last real one delivers sum w (the norm).
// The first pass of each entry point takes sums (means); the second centres on them (two-pass, like the reference) and
// takes the cross products, whose diagonal is the variance: nothing is shifted by a provisional estimate.
// No N x n scratch: the map, the projection and the exp are recomputed from the resident columns in each pass.
// Deterministic: the MFMA accumulation order within a block is fixed, each block writes its own partial tile, and
// k_pca_fin adds the blocks' partials in a fixed order (no floating-point atomics); the chunking depends on N and the CU
// count only.  The n x n finish (division by the norm, square roots, mirroring) runs on the host in fixed order.
#include "ctx.hpp"

#include <cmath>
#include <vector>

#define PCA_KS 32                // rows per slab
#define PCA_KSP (PCA_KS + 2)     // LDS column stride (doubles): 64 distinct banks per half-wave for the operand reads
#define PCA_NT 256               // 4 waves
#define PCA_GT 4                 // tiles per side of a group: a group is a GT x GT rectangle of tile pairs, 4 per wave
#define PCA_LDS_MAX (160 * 1024)

enum { PCA_CORR = 0, PCA_PROJ = 1 };

struct PcaGroup {
    int la, nA;  // left tiles [la, la + nA)
    int rb, nB;  // right tiles [rb, rb + nB); rb = -1: the ones column
    int sym;     // right range == left range of the same space: the right slab is the left one (only a <= b computed)
};

struct PcaArgs {
    const double* cols;
    int64_t ld, N;
    const double* w;        // sample weights (nullptr: unit)
    const int* colidx;      // corr: n columns; proj: np columns
    const int* maps;        // 0 N, 1 L, 2 M
    const double* centre;   // corr: per mapped column (0 in the sums pass); proj: per PC
    const double* zmean;    // proj: mean of the mapped columns
    const double* zsd;      // proj: sd' of the mapped columns (1 where sd = 0)
    const double* U;        // proj: np x np, row c = PC c
    const double* amean;    // proj: base means of the n_all columns
    const double* asd;      // proj: base sddev of the n_all columns
    int nv;                 // real left virtual columns (corr: n, proj: np); column nv is the ones column when `ones`
    int ntp;                // proj: PC tiles of the right space (x tile t >= ntp is column block t - ntp)
    int nall;               // proj: x columns of the right space
    int doexp;
    int ones;               // sums pass
};

__device__ __forceinline__ double pca_map(int m, double x) {
    return m == 0 ? x : (m == 1 ? log(x) : log(-x));
}

// pair e of a group -> (left tile, right tile offset), false when the slot is dead
__device__ __forceinline__ bool pca_pair(const PcaGroup& G, int ones, int e, int& ao, int& bo) {
    if (ones) {
        ao = e, bo = 0;
        return e < G.nA;
    }
    ao = e / PCA_GT, bo = e % PCA_GT;
    return ao < G.nA && bo < G.nB && !(G.sym && ao > bo);
}

// grid (nchunks, ngroups); dynamic LDS: sW[KS] | sL[GT*16][KSP] | sR[GT*16][KSP] | (proj) sZ[np][KSP]
template <int MODE>
__global__ void __launch_bounds__(PCA_NT) k_pca_tiles(PcaArgs A, const PcaGroup* __restrict__ groups, int64_t rows_per_chunk,
                                                      double* __restrict__ part) {
    typedef double f64x4 __attribute__((ext_vector_type(4)));
    extern __shared__ double lds[];
    constexpr int NC = PCA_GT * 16;
    double* sW = lds;
    double* sL = lds + PCA_KS;
    double* sR = sL + NC * PCA_KSP;
    double* sZ = sR + NC * PCA_KSP;
    const PcaGroup G = groups[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lk = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = A.nv;
    f64x4 acc[4];
    int offA[4], offB[4];
    bool live[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int ao, bo;
        live[q] = pca_pair(G, A.ones, wv * 4 + q, ao, bo);
        offA[q] = ao * 16 * PCA_KSP;
        offB[q] = bo * 16 * PCA_KSP;
        acc[q] = (f64x4){0.0, 0.0, 0.0, 0.0};
    }
    const double* sRB = G.sym ? sL : sR;
    const int64_t c_lo = (int64_t)blockIdx.x * rows_per_chunk;
    int64_t c_hi = c_lo + rows_per_chunk;
    if (c_hi > A.N) c_hi = A.N;
    const int nLc = G.nA * 16, nRc = (A.ones || G.sym) ? 0 : G.nB * 16;

    // value of left virtual column c (absolute) at slab row r (row valid)
    auto proj_pc = [&](int c, int r) -> double {
        double s = 0.0;
        const double* u = A.U + (int64_t)c * np;
        for (int k = 0; k < np; ++k) s += u[k] * sZ[k * PCA_KSP + r];
        return A.doexp ? exp(s) : s;
    };
    for (int64_t r0 = c_lo; r0 < c_hi; r0 += PCA_KS) {
        __syncthreads();  // the previous slab's operand reads are done
        if (tid < PCA_KS) {
            const int64_t row = r0 + tid;
            sW[tid] = row < c_hi ? (A.w ? A.w[row] : 1.0) : 0.0;
        }
        if (MODE == PCA_PROJ) {
            for (int e = tid; e < np * PCA_KS; e += PCA_NT) {
                const int k = e / PCA_KS, r = e % PCA_KS;
                const int64_t row = r0 + r;
                double z = 0.0;
                if (row < c_hi) {
                    const double y = pca_map(A.maps[k], A.cols[(int64_t)A.colidx[k] * A.ld + row]);
                    z = (y - A.zmean[k]) / A.zsd[k];
                }
                sZ[k * PCA_KSP + r] = z;
            }
            __syncthreads();
        }
        // left range (and the ones column)
        for (int e = tid; e < nLc * PCA_KS; e += PCA_NT) {
            const int cl = e / PCA_KS, r = e % PCA_KS;
            const int c = G.la * 16 + cl;
            const int64_t row = r0 + r;
            double v = 0.0;
            if (row < c_hi) {
                if (c < A.nv) {
                    if (MODE == PCA_CORR)
                        v = pca_map(A.maps[c], A.cols[(int64_t)A.colidx[c] * A.ld + row]) - A.centre[c];
                    else
                        v = proj_pc(c, r) - A.centre[c];
                } else if (A.ones && c == A.nv) {
                    v = 1.0;
                }
            }
            sL[cl * PCA_KSP + r] = v;
        }
        // right range (its own slab unless it is the left one or the ones column)
        for (int e = tid; e < nRc * PCA_KS; e += PCA_NT) {
            const int cl = e / PCA_KS, r = e % PCA_KS;
            const int t = G.rb + cl / 16;
            const int64_t row = r0 + r;
            double v = 0.0;
            if (row < c_hi) {
                if (MODE == PCA_CORR) {
                    const int c = t * 16 + cl % 16;
                    if (c < A.nv) v = pca_map(A.maps[c], A.cols[(int64_t)A.colidx[c] * A.ld + row]) - A.centre[c];
                } else if (t < A.ntp) {
                    const int c = t * 16 + cl % 16;
                    if (c < A.nv) v = proj_pc(c, r) - A.centre[c];
                } else {
                    const int j = (t - A.ntp) * 16 + cl % 16;
                    if (j < A.nall) v = (A.cols[(int64_t)j * A.ld + row] - A.amean[j]) / A.asd[j];
                }
            }
            sR[cl * PCA_KSP + r] = v;
        }
        __syncthreads();
        const double bones = l15 == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int kk = 0; kk < PCA_KS / 4; ++kk) {
            const double wk = sW[kk * 4 + lk];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!live[q]) continue;  // wave-uniform
                const double a = sL[offA[q] + l15 * PCA_KSP + kk * 4 + lk] * wk;
                const double b = A.ones ? bones : sRB[offB[q] + l15 * PCA_KSP + kk * 4 + lk];
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
            }
        }
    }
    // partial tile of (chunk, group, slot): element (i, j) = (lk + 4 rg, l15), i from the left tile, j from the right
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double* p = part + (((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 16 + wv * 4 + q) * 256;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) p[(lk + 4 * rg) * 16 + l15] = acc[q][rg];
    }
}

// S[slot][e] = sum over chunks of part[chunk][slot][e], chunk order fixed: four interleaved sums combined in a fixed order
__global__ void __launch_bounds__(1024) k_pca_fin(const double* __restrict__ part, int nchunks, int nslots,
                                                  double* __restrict__ S) {
    __shared__ double sh[4][256];
    const int e = threadIdx.x & 255, l4 = threadIdx.x >> 8;
    const double* p = part + (int64_t)blockIdx.x * 256 + e;
    double s = 0.0;
    for (int b = l4; b < nchunks; b += 4) s += p[(int64_t)b * nslots * 256];
    sh[l4][e] = s;
    __syncthreads();
    if (l4 == 0) S[(int64_t)blockIdx.x * 256 + e] = (sh[0][e] + sh[1][e]) + (sh[2][e] + sh[3][e]);
}

namespace {

// groups of a sums pass: left ranges of GT tiles over nv + 1 columns (the ones column last)
std::vector<PcaGroup> pca_sum_groups(int nv) {
    const int nt = (nv + 1 + 15) / 16;
    std::vector<PcaGroup> g;
    for (int a = 0; a < nt; a += PCA_GT) g.push_back({a, nt - a < PCA_GT ? nt - a : PCA_GT, -1, 1, 0});
    return g;
}

// groups of a cross pass: symmetric left x left (upper triangle of ranges), then left x extra right tiles [rt0, rt1)
std::vector<PcaGroup> pca_cross_groups(int ntl, int rt0, int rt1) {
    std::vector<PcaGroup> g;
    for (int a = 0; a < ntl; a += PCA_GT) {
        const int nA = ntl - a < PCA_GT ? ntl - a : PCA_GT;
        for (int b = a; b < ntl; b += PCA_GT) {
            const int nB = ntl - b < PCA_GT ? ntl - b : PCA_GT;
            g.push_back({a, nA, b, nB, a == b ? 1 : 0});
        }
        for (int b = rt0; b < rt1; b += PCA_GT) g.push_back({a, nA, b, rt1 - b < PCA_GT ? rt1 - b : PCA_GT, 0});
    }
    return g;
}

size_t pca_lds_bytes(int mode, int np) {
    return (size_t)(PCA_KS + 2 * PCA_GT * 16 * PCA_KSP + (mode == PCA_PROJ ? np * PCA_KSP : 0)) * 8;
}

// chunks of rows (multiples of KS): about 4 blocks per CU over all groups, at most one slab per chunk row
void pca_chunks(const gd_ctx* ctx, int ngroups, int& nchunks, int64_t& rows) {
    const int64_t N = ctx->N;
    int64_t want = (4LL * ctx->cu_count + ngroups - 1) / ngroups;
    const int64_t most = (N + PCA_KS - 1) / PCA_KS;
    if (want > most) want = most;
    if (want < 1) want = 1;
    rows = (N + want - 1) / want;
    rows = (rows + PCA_KS - 1) / PCA_KS * PCA_KS;
    nchunks = (int)((N + rows - 1) / rows);
}

// one pass: launch over the groups, add the chunks' partials, bring S (ngroups x 16 slots x 256) to the host
int pca_pass(gd_ctx* ctx, int mode, const PcaArgs& A, const std::vector<PcaGroup>& groups, PcaGroup* d_groups,
             double* d_part, int64_t part_cap, double* d_S, std::vector<double>& S) {
    const int ng = (int)groups.size();
    int nchunks;
    int64_t rows;
    pca_chunks(ctx, ng, nchunks, rows);
    if ((int64_t)nchunks * ng * 16 * 256 > part_cap) return gd_fail(ctx, GD_ERR_NOMEM, "pca: partial buffer too small");
    GD_TRY(gd_h2d(ctx, d_groups, groups.data(), groups.size() * sizeof(PcaGroup)));
    const size_t lds = pca_lds_bytes(mode, A.nv);
    if (mode == PCA_CORR) {
        GD_HIP(hipFuncSetAttribute((const void*)k_pca_tiles<PCA_CORR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_pca_tiles<PCA_CORR><<<dim3(nchunks, ng), PCA_NT, lds, ctx->stream>>>(A, d_groups, rows, d_part);
    } else {
        GD_HIP(hipFuncSetAttribute((const void*)k_pca_tiles<PCA_PROJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_pca_tiles<PCA_PROJ><<<dim3(nchunks, ng), PCA_NT, lds, ctx->stream>>>(A, d_groups, rows, d_part);
    }
    GD_KERNEL_CHECK();
    k_pca_fin<<<ng * 16, 1024, 0, ctx->stream>>>(d_part, nchunks, ng * 16, d_S);
    GD_KERNEL_CHECK();
    S.assign((size_t)ng * 16 * 256, 0.0);
    GD_TRY(gd_fetch(ctx, S.data(), d_S, S.size() * 8));
    return gd_stream_sync(ctx);
}

// element (i, j) of the product of left tile a and right tile b from a cross pass's S, or false when no slot holds it
struct PcaIndex {
    std::vector<int> slot;  // [a * ntr + b] -> slot, -1 when not computed
    int ntr;
};
PcaIndex pca_index(const std::vector<PcaGroup>& groups, int ntl, int ntr) {
    PcaIndex ix{std::vector<int>((size_t)ntl * ntr, -1), ntr};
    for (size_t g = 0; g < groups.size(); ++g)
        for (int e = 0; e < 16; ++e) {
            const PcaGroup& G = groups[g];
            const int ao = e / PCA_GT, bo = e % PCA_GT;
            if (ao < G.nA && bo < G.nB && !(G.sym && ao > bo)) ix.slot[(size_t)(G.la + ao) * ntr + G.rb + bo] = (int)g * 16 + e;
        }
    return ix;
}
inline double pca_at(const std::vector<double>& S, const PcaIndex& ix, int i, int j) {
    const int s = ix.slot[(size_t)(i / 16) * ix.ntr + j / 16];
    return S[(size_t)s * 256 + (i % 16) * 16 + j % 16];
}
// column sums of a sums pass: virtual column c
inline double pca_sum(const std::vector<double>& S, int c) {
    const int t = c / 16, g = t / PCA_GT, e = t % PCA_GT;
    return S[((size_t)g * 16 + e) * 256 + (c % 16) * 16];
}

struct PcaScratch {
    int* colidx;
    int* maps;
    double *centre, *zmean, *zsd, *U, *amean, *asd;
    PcaGroup* groups;
    double *part, *S;
    int64_t part_cap;
};

// one scratch block for both passes of a call: tables, group descriptors, S and the partials (max_slots = the larger
// chunks x groups of the two passes)
int pca_scratch(gd_ctx* ctx, int nc, int np, int nall, int max_groups, int64_t max_slots, PcaScratch& sc) {
    sc.part_cap = max_slots * 16 * 256;
    ScratchPlan sp;
    auto colidx = sp.take<int>(nc), maps = sp.take<int>(nc);
    auto centre = sp.take<double>(nc + 1), zmean = sp.take<double>(nc), zsd = sp.take<double>(nc);
    auto U = sp.take<double>((int64_t)np * np + 1), amean = sp.take<double>(nall + 1), asd = sp.take<double>(nall + 1);
    auto groups = sp.take<PcaGroup>(max_groups);
    auto S = sp.take<double>((int64_t)max_groups * 16 * 256), part = sp.take<double>(sc.part_cap);
    GD_TRY(sp.get(ctx));
    sc.colidx = colidx, sc.maps = maps, sc.centre = centre, sc.zmean = zmean, sc.zsd = zsd, sc.U = U;
    sc.amean = amean, sc.asd = asd, sc.groups = groups, sc.S = S, sc.part = part;
    return GD_OK;
}

int pca_check(gd_ctx* ctx, const int32_t* cols, int32_t n, const int32_t* maps) {
    GD_REQUIRE(ctx && cols && maps, "null argument");
    GD_REQUIRE(ctx->cols && ctx->N > 0, "no samples uploaded (empty row range)");
    GD_REQUIRE(n >= 1 && n <= ctx->n, "number of PCA columns out of range (1..uploaded columns)");
    GD_REQUIRE_SAMPLE_COLUMNS(cols, n);
    for (int i = 0; i < n; ++i) GD_REQUIRE(maps[i] >= 0 && maps[i] <= 2, "PCA map must be 0 (N), 1 (L) or 2 (M)");
    return GD_OK;
}

int64_t pca_max_slots(const gd_ctx* ctx, const std::vector<std::vector<PcaGroup>*>& plans) {
    int64_t mx = 1;
    for (auto* g : plans) {
        int nchunks;
        int64_t rows;
        pca_chunks(ctx, (int)g->size(), nchunks, rows);
        const int64_t slots = (int64_t)nchunks * (int64_t)g->size();
        if (slots > mx) mx = slots;
    }
    return mx;
}

}  // namespace

extern "C" {

int gd_pca_corr(gd_ctx* ctx, const int32_t* cols, int32_t n, const int32_t* maps, double* mean_out, double* sd_out,
                double* corr_out) {
    GD_TRY(pca_check(ctx, cols, n, maps));
    GD_REQUIRE(mean_out && sd_out && corr_out, "null output");
    const double* w = ctx->w_sel ? ctx->w_main : ctx->w;  // always the sample weights
    std::vector<PcaGroup> g1 = pca_sum_groups(n);
    const int ntl = (n + 15) / 16;
    std::vector<PcaGroup> g2 = pca_cross_groups(ntl, 0, 0);
    const int maxg = (int)(g1.size() > g2.size() ? g1.size() : g2.size());
    PcaScratch sc;
    GD_TRY(pca_scratch(ctx, n, 0, 0, maxg, pca_max_slots(ctx, {&g1, &g2}), sc));
    GD_TRY(gd_h2d(ctx, sc.colidx, cols, (size_t)n * 4));
    GD_TRY(gd_h2d(ctx, sc.maps, maps, (size_t)n * 4));
    GD_HIP(hipMemsetAsync(sc.centre, 0, (size_t)(n + 1) * 8, ctx->stream));
    PcaArgs A{};
    A.cols = ctx->cols, A.ld = ctx->ld, A.N = ctx->N, A.w = w, A.colidx = sc.colidx, A.maps = sc.maps, A.centre = sc.centre;
    A.nv = n, A.ones = 1;
    std::vector<double> S;
    GD_TRY(pca_pass(ctx, PCA_CORR, A, g1, sc.groups, sc.part, sc.part_cap, sc.S, S));
    const double norm = pca_sum(S, n);
    std::vector<double> mean((size_t)n), sdp((size_t)n);
    for (int c = 0; c < n; ++c) mean[c] = pca_sum(S, c) / norm;
    GD_TRY(gd_h2d(ctx, sc.centre, mean.data(), (size_t)n * 8));
    A.ones = 0;
    GD_TRY(pca_pass(ctx, PCA_CORR, A, g2, sc.groups, sc.part, sc.part_cap, sc.S, S));
    const PcaIndex ix = pca_index(g2, ntl, ntl);
    for (int c = 0; c < n; ++c) {
        mean_out[c] = mean[c];
        sd_out[c] = sqrt(pca_at(S, ix, c, c) / norm);
        sdp[c] = sd_out[c] != 0 ? sd_out[c] : 1.0;
    }
    for (int i = 0; i < n; ++i) {
        corr_out[(int64_t)i * n + i] = 1.0;  // by construction (never computed, like the reference)
        for (int j = i + 1; j < n; ++j) {
            const double v = pca_at(S, ix, i, j) / sdp[i] / sdp[j] / norm;
            corr_out[(int64_t)i * n + j] = v;
            corr_out[(int64_t)j * n + i] = v;
        }
    }
    return GD_OK;
}

int gd_pca_project(gd_ctx* ctx, const int32_t* cols, int32_t np, const int32_t* maps, const double* mean, const double* sd,
                   const double* U, int32_t doexp, int32_t n_all, const double* all_means, const double* all_sd,
                   double* newmean_out, double* newsd_out, double* pcpc_out, double* pcpar_out) {
    GD_TRY(pca_check(ctx, cols, np, maps));
    GD_REQUIRE(mean && sd && U && all_means && all_sd, "null input");
    GD_REQUIRE(newmean_out && newsd_out && pcpc_out && pcpar_out, "null output");
    GD_REQUIRE(n_all >= 1 && n_all <= ctx->n, "n_all out of range (1..uploaded columns)");
    GD_REQUIRE(np <= GD_PCA_MAX_PROJ && pca_lds_bytes(PCA_PROJ, np) <= PCA_LDS_MAX,
               "too many PCA parameters for one projection (GD_PCA_MAX_PROJ)");
    const double* w = ctx->w_sel ? ctx->w_main : ctx->w;
    const int ntp = (np + 15) / 16, ntx = (n_all + 15) / 16;
    std::vector<PcaGroup> g1 = pca_sum_groups(np);
    std::vector<PcaGroup> g2 = pca_cross_groups(ntp, ntp, ntp + ntx);
    const int maxg = (int)(g1.size() > g2.size() ? g1.size() : g2.size());
    PcaScratch sc;
    GD_TRY(pca_scratch(ctx, np, np, n_all, maxg, pca_max_slots(ctx, {&g1, &g2}), sc));
    std::vector<double> sdp((size_t)np);
    for (int k = 0; k < np; ++k) sdp[k] = sd[k] != 0 ? sd[k] : 1.0;
    GD_TRY(gd_h2d(ctx, sc.colidx, cols, (size_t)np * 4));
    GD_TRY(gd_h2d(ctx, sc.maps, maps, (size_t)np * 4));
    GD_TRY(gd_h2d(ctx, sc.zmean, mean, (size_t)np * 8));
    GD_TRY(gd_h2d(ctx, sc.zsd, sdp.data(), (size_t)np * 8));
    GD_TRY(gd_h2d(ctx, sc.U, U, (size_t)np * np * 8));
    GD_TRY(gd_h2d(ctx, sc.amean, all_means, (size_t)n_all * 8));
    GD_TRY(gd_h2d(ctx, sc.asd, all_sd, (size_t)n_all * 8));
    GD_HIP(hipMemsetAsync(sc.centre, 0, (size_t)(np + 1) * 8, ctx->stream));
    PcaArgs A{};
    A.cols = ctx->cols, A.ld = ctx->ld, A.N = ctx->N, A.w = w, A.colidx = sc.colidx, A.maps = sc.maps, A.centre = sc.centre;
    A.zmean = sc.zmean, A.zsd = sc.zsd, A.U = sc.U, A.amean = sc.amean, A.asd = sc.asd;
    A.nv = np, A.ntp = ntp, A.nall = n_all, A.doexp = doexp ? 1 : 0, A.ones = 1;
    std::vector<double> S;
    GD_TRY(pca_pass(ctx, PCA_PROJ, A, g1, sc.groups, sc.part, sc.part_cap, sc.S, S));
    const double norm = pca_sum(S, np);
    for (int i = 0; i < np; ++i) newmean_out[i] = pca_sum(S, i) / norm;
    GD_TRY(gd_h2d(ctx, sc.centre, newmean_out, (size_t)np * 8));
    A.ones = 0;
    GD_TRY(pca_pass(ctx, PCA_PROJ, A, g2, sc.groups, sc.part, sc.part_cap, sc.S, S));
    const PcaIndex ix = pca_index(g2, ntp, ntp + ntx);
    for (int i = 0; i < np; ++i) newsd_out[i] = sqrt(pca_at(S, ix, i, i) / norm);
    for (int i = 0; i < np; ++i) {
        for (int j = i; j < np; ++j) {
            const double v = pca_at(S, ix, i, j) / newsd_out[i] / newsd_out[j] / norm;
            pcpc_out[(int64_t)i * np + j] = v;
            pcpc_out[(int64_t)j * np + i] = v;
        }
        for (int j = 0; j < n_all; ++j) pcpar_out[(int64_t)i * n_all + j] = pca_at(S, ix, i, ntp * 16 + j) / newsd_out[i] / norm;
    }
    return GD_OK;
}

}  // extern "C"
