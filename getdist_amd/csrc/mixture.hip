// Gaussian-mixture log-pdf over the resident sample rows (gaussian_mixtures.MixtureND.logLikes / MCSamples(logLikes=True)).
//
//   out[r] = -log sum_k exp(logcoef_k - 1/2 |W_k (x_r - mu_k)|^2),   W_k = L_k^-1 lower-triangular, cov_k = L_k L_k^T
//
// A block owns BR = G * RG consecutive rows.  It stages the d selected columns of those rows ONCE in LDS (sX[j][BR], the
// only read of the samples: every component works from the staged tile), then each wave evaluates "units": unit (k, I) is
// the 16 rows [16 I, 16 I + 16) of y = W_k (x - mu_k) for one component.  A lane is a sample row; the unit keeps its 16 y
// values in registers and walks the column blocks J <= I, 8 staged x values at a time (registers: 16 + 8 doubles,
// whatever d is -- a large d is more column blocks, not more registers).  W and mu are indexed by wave-uniform counters
// only, so the compiler reads them through the scalar cache and every product is one v_fma_f64 with an SGPR operand.
// The S waves that share a row group split the K * ceil(d / 16) units by a host-made table (longest unit first onto the
// least loaded wave, each wave's list in ascending order); with S > 1 the per-component partial sums of squares meet in
// LDS (sQ[s][k][BR]) and wave 0 of the group adds them in wave order.  The sum over components is a running max-shifted
// log-sum-exp, so a row 40 sigma out stays finite.
// Deterministic: the order of every sum is a function of (d, K) alone -- columns ascending within a y_i, i ascending
// within a unit, units ascending within a wave, waves ascending, components ascending.  No atomics, no N x d temporary:
// the only O(N) write is the result vector.
#include "ctx.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#define MIX_B 16                     // rows / columns of a block of W
#define MIX_LDS_MAX (160 * 1024)
#define MIX_LDS_PREF (64 * 1024)     // at least two blocks per CU

struct MixArgs {
    const double* cols;
    int64_t ld, lo, hi;
    const int* colidx;       // d
    const double* W;         // K x dp x dp, rows and columns zero-padded to dp = 16 ceil(d / 16)
    const double* mu;        // K x dp
    const double* logcoef;   // K
    const int* units;        // S x (ucap + 1): count, then codes k * nI + I ascending
    int d, dp, K, nI;
    int G, S, RG, brs;       // row groups per block, waves per group, rows per group, log2(G * RG)
    int ucap;
    double* out;             // hi - lo
};

// sum of squares of rows [16 I, 16 I + 4 N4) of W_k (x - mu_k) for the lane's sample row; xs = the row's column 0 in sX
template <int N4>
__device__ __forceinline__ double mix_unit(const double* __restrict__ Wk, const double* __restrict__ muk, const double* xs,
                                           int BR, int I, int d, int dp) {
    double acc[4 * N4];
#pragma unroll
    for (int i = 0; i < 4 * N4; ++i) acc[i] = 0.0;
    const int i0 = I * MIX_B;
    for (int jb = 0; jb < I; ++jb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j0 = jb * MIX_B + h * 8;
            double dx[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) dx[jj] = xs[(j0 + jj) * BR] - muk[j0 + jj];
#pragma unroll
            for (int i = 0; i < 4 * N4; ++i) {
                const double* w = Wk + (int64_t)(i0 + i) * dp + j0;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) acc[i] = __builtin_fma(w[jj], dx[jj], acc[i]);
            }
        }
    }
    // the diagonal block: columns i0 .. i0 + i of row i0 + i (columns at or beyond d are padding)
    double dx[4 * N4];
#pragma unroll
    for (int jj = 0; jj < 4 * N4; ++jj) {
        const int j = i0 + jj;
        dx[jj] = j < d ? xs[j * BR] - muk[j] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4 * N4; ++i) {
        const double* w = Wk + (int64_t)(i0 + i) * dp + i0;
#pragma unroll
        for (int jj = 0; jj <= i; ++jj) acc[i] = __builtin_fma(w[jj], dx[jj], acc[i]);
    }
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 4 * N4; ++i) q = __builtin_fma(acc[i], acc[i], q);
    return q;
}

// running log-sum-exp: sum_k exp(t_k) = ssum * exp(m)
__device__ __forceinline__ void mix_lse(double t, double& m, double& ssum) {
    if (t != t) {
        ssum = t;
    } else if (t > m) {
        ssum = ssum * exp(m - t) + 1.0;
        m = t;
    } else if (t > -INFINITY) {
        ssum += exp(t - m);
    }
}

// grid: ceil((hi - lo) / BR) blocks of 64 G S threads; dynamic LDS: sX[d][BR] | sQ[S][K][BR] (S > 1)
__global__ void __launch_bounds__(256) k_mixture_nll(MixArgs A) {
    extern __shared__ double lds[];
    const int BR = 1 << A.brs;
    double* sX = lds;
    double* sQ = lds + (int64_t)A.d * BR;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wv / A.S, s = wv - g * A.S;
    const int64_t r0 = A.lo + (int64_t)blockIdx.x * BR;
    const int nthr = 64 * A.G * A.S;
    const int total = A.d << A.brs;
#pragma unroll 4
    for (int e = tid; e < total; e += nthr) {
        const int j = e >> A.brs, r = e & (BR - 1);
        const int64_t row = r0 + r;
        sX[e] = row < A.hi ? A.cols[(int64_t)A.colidx[j] * A.ld + row] : 0.0;
    }
    const bool live = lane < A.RG;
    const int rl = g * A.RG + (live ? lane : 0);  // the lane's row within the block (idle lanes shadow row 0 of the group)
    if (A.S > 1)
        for (int k = 0; k < A.K; ++k) sQ[((int64_t)s * A.K + k) * BR + rl] = 0.0;
    __syncthreads();

    const double* xs = sX + rl;
    const int* ul = A.units + s * (A.ucap + 1);
    const int nu = __builtin_amdgcn_readfirstlane(ul[0]);
    double m = -INFINITY, ssum = 0.0, q = 0.0;
    int kcur = -1;
    for (int u = 0; u < nu; ++u) {
        const int code = __builtin_amdgcn_readfirstlane(ul[1 + u]);
        const int k = code / A.nI, I = code - k * A.nI;
        if (k != kcur) {
            if (kcur >= 0) {
                if (A.S > 1)
                    sQ[((int64_t)s * A.K + kcur) * BR + rl] = q;
                else
                    mix_lse(A.logcoef[kcur] - 0.5 * q, m, ssum);
            }
            kcur = k, q = 0.0;
        }
        const double* Wk = A.W + (int64_t)k * A.dp * A.dp;
        const double* muk = A.mu + (int64_t)k * A.dp;
        int n4 = (A.d - I * MIX_B + 3) >> 2;
        double qu;
        if (n4 >= 4)
            qu = mix_unit<4>(Wk, muk, xs, BR, I, A.d, A.dp);
        else if (n4 == 3)
            qu = mix_unit<3>(Wk, muk, xs, BR, I, A.d, A.dp);
        else if (n4 == 2)
            qu = mix_unit<2>(Wk, muk, xs, BR, I, A.d, A.dp);
        else
            qu = mix_unit<1>(Wk, muk, xs, BR, I, A.d, A.dp);
        q += qu;
    }
    if (kcur >= 0) {
        if (A.S > 1)
            sQ[((int64_t)s * A.K + kcur) * BR + rl] = q;
        else
            mix_lse(A.logcoef[kcur] - 0.5 * q, m, ssum);
    }
    if (A.S > 1) {
        __syncthreads();
        if (s != 0) return;
        for (int k = 0; k < A.K; ++k) {
            double qk = 0.0;
            for (int t = 0; t < A.S; ++t) qk += sQ[((int64_t)t * A.K + k) * BR + rl];
            mix_lse(A.logcoef[k] - 0.5 * qk, m, ssum);
        }
    }
    const int64_t row = r0 + rl;
    if (live && row < A.hi) A.out[row - A.lo] = -(m + log(ssum));
}

namespace {

struct MixPlan {
    int G, S, RG;
    size_t lds;
};

size_t mix_lds_bytes(int d, int K, int G, int S, int RG) {
    return (size_t)8 * ((size_t)d * G * RG + (S > 1 ? (size_t)S * K * G * RG : 0));
}

// waves per row group (S <= the number of units), row groups per block (G S <= 4) and rows per group: the widest split
// that leaves two blocks per CU; failing that anything that fits, a full wave of rows first
bool mix_plan(int d, int K, MixPlan& P) {
    const int64_t units = (int64_t)K * ((d + MIX_B - 1) / MIX_B);
    int smax = 1;
    while (smax * 2 <= 4 && smax * 2 <= units) smax *= 2;
    for (int pass = 0; pass < 2; ++pass) {
        const size_t cap = pass ? MIX_LDS_MAX : MIX_LDS_PREF;
        for (int RG = 64; RG >= (pass ? 16 : 64); RG /= 2)
            for (int S = smax; S >= 1; S /= 2)
                for (int G = 4 / S; G >= 1; G /= 2) {
                    const size_t b = mix_lds_bytes(d, K, G, S, RG);
                    if (b <= cap) {
                        P = {G, S, RG, b};
                        return true;
                    }
                }
    }
    return false;
}

// units dealt to the S waves of a row group: by decreasing cost onto the least loaded wave (ties: the lower wave), then
// each wave's list ascending.  table: S x (ucap + 1) = count, codes
void mix_units(int d, int K, int S, std::vector<int>& table, int& ucap) {
    const int nI = (d + MIX_B - 1) / MIX_B;
    struct U {
        int code;
        int64_t cost;
    };
    std::vector<U> us;
    for (int k = 0; k < K; ++k)
        for (int I = 0; I < nI; ++I) {
            const int rows = std::min(MIX_B, (d - I * MIX_B + 3) / 4 * 4);
            us.push_back({k * nI + I, (int64_t)rows * (MIX_B * I) + (int64_t)rows * (rows + 1) / 2});
        }
    std::stable_sort(us.begin(), us.end(), [](const U& a, const U& b) { return a.cost > b.cost; });
    std::vector<std::vector<int>> lists((size_t)S);
    std::vector<int64_t> load((size_t)S, 0);
    for (const U& u : us) {
        int best = 0;
        for (int s = 1; s < S; ++s)
            if (load[s] < load[best]) best = s;
        lists[best].push_back(u.code);
        load[best] += u.cost;
    }
    ucap = 0;
    for (auto& l : lists) {
        std::sort(l.begin(), l.end());
        ucap = std::max(ucap, (int)l.size());
    }
    table.assign((size_t)S * (ucap + 1), 0);
    for (int s = 0; s < S; ++s) {
        table[(size_t)s * (ucap + 1)] = (int)lists[s].size();
        std::copy(lists[s].begin(), lists[s].end(), table.begin() + (size_t)s * (ucap + 1) + 1);
    }
}

}  // namespace

extern "C" {

int gd_mixture_nll(gd_ctx* ctx, const int32_t* cols, int32_t d, int32_t K, const double* means, const double* whiten,
                   const double* logcoef, int64_t row_lo, int64_t row_hi, double* out) {
    GD_REQUIRE(ctx && cols && means && whiten && logcoef && out, "null argument");
    GD_REQUIRE(ctx->cols && ctx->N > 0, "no samples uploaded (empty row range)");
    GD_REQUIRE(d >= 1 && d <= ctx->n, "mixture dimension out of range (1..uploaded columns)");
    GD_REQUIRE(K >= 1 && (int64_t)K * ((d + MIX_B - 1) / MIX_B) < (1 << 30), "number of mixture components out of range");
    GD_REQUIRE_ROWS(row_lo, row_hi);
    GD_REQUIRE_SAMPLE_COLUMNS(cols, d);
    MixPlan P;
    GD_REQUIRE(mix_plan(d, K, P), "mixture dimension too large for one tile of rows in LDS");
    const int nI = (d + MIX_B - 1) / MIX_B, dp = nI * MIX_B;
    std::vector<int> table;
    int ucap;
    mix_units(d, K, P.S, table, ucap);

    // one host block: W (padded) | mu (padded) | logcoef | colidx | units
    ScratchPlan sp;
    auto d_W = sp.take<double>((int64_t)K * dp * dp);
    auto d_mu = sp.take<double>((int64_t)K * dp);
    auto d_lc = sp.take<double>(K);
    auto d_ci = sp.take<int>(d);
    auto d_u = sp.take<int>((int64_t)table.size());
    const int64_t tab_bytes = sp.bytes();
    const int64_t n = row_hi - row_lo;
    auto d_out = sp.take<double>(n);
    std::vector<char> host((size_t)tab_bytes, 0);
    double* hW = (double*)(host.data() + d_W.off);
    double* hmu = (double*)(host.data() + d_mu.off);
    for (int k = 0; k < K; ++k) {
        for (int i = 0; i < d; ++i) {
            for (int j = 0; j <= i; ++j) hW[((int64_t)k * dp + i) * dp + j] = whiten[((int64_t)k * d + i) * d + j];
            hmu[(int64_t)k * dp + i] = means[(int64_t)k * d + i];
        }
    }
    memcpy(host.data() + d_lc.off, logcoef, (size_t)K * 8);
    memcpy(host.data() + d_ci.off, cols, (size_t)d * 4);
    memcpy(host.data() + d_u.off, table.data(), table.size() * 4);
    GD_TRY(sp.get(ctx));
    GD_TRY(gd_h2d(ctx, d_W, host.data(), (size_t)tab_bytes));

    MixArgs A{};
    A.cols = ctx->cols, A.ld = ctx->ld, A.lo = row_lo, A.hi = row_hi;
    A.colidx = d_ci, A.W = d_W, A.mu = d_mu, A.logcoef = d_lc, A.units = d_u;
    A.d = d, A.dp = dp, A.K = K, A.nI = nI, A.G = P.G, A.S = P.S, A.RG = P.RG, A.ucap = ucap;
    const int BR = P.G * P.RG;
    A.brs = 0;
    while ((1 << A.brs) < BR) ++A.brs;
    A.out = d_out;
    const int64_t nblocks = (n + BR - 1) / BR;
    GD_REQUIRE(nblocks <= 0x7fffffffLL, "row range too long for one launch");
    GD_HIP(hipFuncSetAttribute((const void*)k_mixture_nll, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds));
    k_mixture_nll<<<dim3((unsigned)nblocks), 64 * P.G * P.S, P.lds, ctx->stream>>>(A);
    GD_KERNEL_CHECK();
    // the result goes out on the copy stream behind the kernel; the (pageable) table block stays alive until it has landed
    GD_TRY(gd_memcpy_d2h_async(ctx, out, A.out, n * 8));
    GD_TRY(gd_copy_sync(ctx));
    return GD_OK;
}

}  // extern "C"
