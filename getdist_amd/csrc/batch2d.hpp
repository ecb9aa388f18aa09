// batch2d.hpp -- the host side of gd_density2d_batch: every decision MCSamples.get2DDensityGridData and
// getAutoBandwidth2D make for a batch of parameter pairs (/root/reference/getdist/mcsamples.py:1285-1419, 1486-1498,
// 1748-2010; chains.py:477-574 for the effective sample numbers), in the reference's own expression order, plus the
// choreography of the device work over two streams.
//
// Pure C++17, no HIP: the device is reached through a table of entry points (`Ops`).  libgdhip.so binds the table to its
// own C ABI (batch2d.hip); the CPU test-suite binds it to callbacks of the numpy context double and checks the grids of
// this orchestration against the Python-planned path (tests/native/batch_harness.cpp, tests/test_native_batch.py).
//
// Scalars that decide bits downstream (bin edges, shear coefficients, fallback times, window sizes) are evaluated with
// exactly the operations numpy / CPython perform: libm `pow` where Python writes `**` on scalars, x*x where numpy
// squares an array, round-half-even where numpy rounds, the LAPACK 2 x 2 factorisations spelled out (`chol_shear`).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/gdhip.h"

namespace gdb {

// ---- device entry points (the C ABI of include/gdhip.h, handle first) -------------------------------------------------
struct Ops {
    int (*bind_thread)(void* h);
    int (*num_rows)(void* h, int64_t* N, int64_t* n);
    int (*weights_kind)(void* h, int32_t* has_weights);  // 0: unit weights (chains.py:313-315), 1: weights, 2: real weights
                                                         //    whose byte-index binning the library serves (sorted by stripe)
    int (*dev_alloc)(void* h, int64_t bytes, void** out);
    int (*dev_free)(void* h, void* p);
    int (*prebin8_batch)(void* h, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, int32_t F,
                         void* const* d_idx, int64_t* bad);
    int (*hist2d_prebinned8)(void* h, int32_t B, const void* const* ix, const void* const* iy, void* d_hist);
    // both of the above back to back with one wait (ncols may be 0); GD_ERR_SOLVER: a sample outside the grid or a wrapped counter
    int (*prebin8_hist2d)(void* h, const int32_t* cols, int32_t ncols, const double* binmin, const double* width,
                          void* const* d_idx, int64_t* bad, int32_t B, const void* const* ix, const void* const* iy, void* d_hist);
    int (*prebin)(void* h, int32_t col, double binmin, double width, int32_t F, void* d_idx);
    int (*hist2d_prebinned)(void* h, int32_t B, const void* const* ix, const void* const* iy, int32_t F, void* d_hist);
    int (*minmax_affine)(void* h, int32_t B, const int32_t* ci, const int32_t* cj, const double* a, const double* b, double* out);
    int (*hist2d_sheared)(void* h, int32_t B, const int32_t* ci, const int32_t* cj, const double* r0, const double* r1,
                          const double* xmin, const double* dx, const double* ymin, const double* dy, int32_t F, void* d_hist);
    int (*kopt2d)(void* h, int32_t B, int32_t F, const void* d_hist, const double* neff, const int32_t* do_corr,
                  const double* fallback_t, const double* corr, double* out);
    // d_dst[(dst_first + k)] = d_src[index[k]], items of item_bytes
    int (*gather_items)(void* h, void* d_dst, int64_t dst_first, const void* d_src, const int32_t* index, int32_t count,
                        int64_t item_bytes);
    // hist_index (may be null: the batch is d_hist's first B grids): pair b convolves histogram hist_index[b] of d_hist
    int (*density2d_enqueue)(void* h, int32_t B, int32_t F, const void* d_hist, const int32_t* hist_index, const double* rx,
                             const double* ry, const double* corr, const int32_t* winw, const int32_t* flags, int32_t bco,
                             int32_t mbc, void* d_P, int32_t* status_pinned);
    int (*d2h_async)(void* h, void* dst, const void* d_src, int64_t bytes);
    int (*copy_mark)(void* h, int32_t* token);
    int (*copy_wait)(void* h, int32_t token);
    int (*copy_sync)(void* h);
    int (*contour_levels)(void* h, int32_t B, int32_t F, const void* d_P, const double* contours, int32_t nc, double* out,
                          int32_t* status);
    int (*autocov_lags_batch)(void* h, const int32_t* cols, int32_t ncols, const double* means, int64_t k0, int32_t nlags,
                              double* out);
    int (*kde_lag_sums_batch)(void* h, const int32_t* cols, int32_t ncols, const double* inv4s2, const int64_t* lags,
                              int32_t nlags, double* out);
    int (*kde_lag_sums)(void* h, int32_t col, double inv4s2, const int64_t* lags, int32_t nlags, double* out);
    const char* (*last_error)(void* h);
    // a further context on h's device over the same resident samples (its own stream and scratch) / its end
    int (*create_aux)(void* h, void** aux);
    int (*destroy_aux)(void* aux);
    // gd_kopt2d in two stream-ordered stages (gdhip.h): everything up to the functionals on h's stream, returning at once;
    // get_h for those rows on ANOTHER context's stream behind the ticket, blocking until the rows are on the host
    int (*kopt2d_enqueue)(void* h, int32_t B, int32_t F, const void* d_hist, const double* neff, const int32_t* do_corr,
                          const double* fallback_t, const double* corr, void* d_rows, int32_t* ticket);
    int (*kopt2d_finish)(void* h, void* stage_a_h, int32_t ticket, int32_t B, void* d_rows, double* out);
    // the context's communicator (gd_comm_init): number of ranks (0: none) / sum all-reduce of a host vector
    int (*comm_world)(void* h);
    int (*comm_allreduce_sum)(void* h, double* inout, int64_t count);
    // the (idle) context's stream re-created with high (1) / normal (0) / low (-1) priority.  The call itself no longer uses it
    // (create_aux gives its contexts their priority); the slot stays so that the table keeps the layout its binders know
    int (*stream_priority)(void* ctx, int level);
    // u16 index columns of several sample columns in ONE launch (gd_prebin_batch; blocking).  May be null: `prebin` per column
    int (*prebin_batch)(void* h, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, int32_t F,
                        void* const* d_idx);
};

// ---- numpy / CPython scalar semantics --------------------------------------------------------------------------------
// `x ** y` on Python floats and numpy float64 scalars is libm pow(x, y).  The exponent goes through a volatile so that
// no compiler rewrites pow(x, 2.0) as x * x (glibc's pow is not correctly rounded in every case; numpy ARRAY squares,
// written x * x below, are).
static inline double py_pow(double x, double y) {
    volatile double e = y;
    return pow(x, e);
}
static inline double np_minimum(double a, double b) { return (a < b || isnan(a)) ? a : b; }
static inline double np_maximum(double a, double b) { return (a > b || isnan(a)) ? a : b; }
static inline double np_sign(double x) { return isnan(x) ? x : (x > 0 ? 1.0 : (x < 0 ? -1.0 : 0.0)); }

// Smallest 2^a * {1,3,5,9,15} (a >= 4) >= n: the frame ladder of the convolution (density2d.hip).
static inline int frame_size(int n) {
    long long best = 1LL << 40;
    const int odd[5] = {1, 3, 5, 9, 15};
    for (int a = 4; a < 28; ++a)
        for (int q = 0; q < 5; ++q) {
            const long long v = (1LL << a) * odd[q];
            if (v >= n && v < best) best = v;
        }
    return (int)best;
}

// np.linalg.cholesky + np.linalg.inv of a 2 x 2 covariance exactly as LAPACK (OpenBLAS potrf / getrf + getrs)
// evaluates them -- reciprocal scaling of the sub-diagonal, partial pivoting in the inverse -- followed by
// mcsamples.py:1352-1356: S *= ichol[0,0]; r = ichol[1,:] / ichol[0,0].  Checked against numpy on random matrices
// (tests/test_native_batch.py).  Returns false when the matrix is not positive definite (numpy raises LinAlgError).
static inline bool chol_shear(double c00, double c10, double c11, double S[4], double r[2]) {
    if (!(c00 > 0)) return false;
    const double l00 = sqrt(c00);
    const double l10 = c10 * (1.0 / l00);
    const double d = c11 - l10 * l10;
    if (!(d > 0)) return false;
    const double l11 = sqrt(d);
    double i00, i10, i11;
    if (fabs(l10) > fabs(l00)) {  // row interchange in dgetrf
        const double l = l00 * (1.0 / l10);
        const double u11 = 0.0 - l * l11;
        i10 = 1.0 * (1.0 / u11);
        i00 = (0.0 - l11 * i10) * (1.0 / l10);
        i11 = (0.0 - l * 1.0) * (1.0 / u11);
    } else {
        const double l = l10 * (1.0 / l00);
        i00 = 1.0 * (1.0 / l00);
        i10 = (0.0 - l * 1.0) * (1.0 / l11);
        i11 = 1.0 * (1.0 / l11);
    }
    S[0] = l00 * i00, S[1] = 0.0 * i00, S[2] = l10 * i00, S[3] = l11 * i00;
    r[0] = i10 / i00, r[1] = i11 / i00;
    return true;
}

// ---- per-pair scalars of get2DDensityGridData (mcsamples.py:1794-1822) ----------------------------------------------
struct PairScalars {
    std::vector<int32_t> jx, jy, F, warn;
    std::vector<int64_t> nbin2D;
    std::vector<double> actual, corr;
};

static inline void pair_scalars(const gd_batch2d_settings& s, int n, const double* corrmat, const int32_t* pairs, int P,
                                PairScalars& ps) {
    ps.jx.resize(P), ps.jy.resize(P), ps.F.resize(P), ps.warn.assign(P, 0), ps.nbin2D.resize(P), ps.actual.resize(P),
        ps.corr.resize(P);
    const int base_F = s.fine_bins_2D;
    for (int k = 0; k < P; ++k) {
        const int a = pairs[2 * k], b = pairs[2 * k + 1];
        ps.jx[k] = a, ps.jy[k] = b;
        const double actual = corrmat[(size_t)b * n + a];  // correlationMatrix[j2, j]
        double c = actual;
        if (fabs(fabs(c) - 1.0) <= 1e-8) {  // "Parameters are 100% correlated" (mcsamples.py:1798-1803)
            ps.warn[k] |= 1;
            c = np_sign(c) * s.max_corr_2D;
        }
        if (fabs(c) < 0.1) c = 0.0;
        const double m = np_minimum(s.max_corr_2D, fabs(c));
        const double angle_scale = np_maximum(0.2, sqrt(1 - m * m));
        ps.nbin2D[k] = (int64_t)nearbyint((double)s.num_bins_2D / angle_scale);
        const int64_t scaled = 192 * (int64_t)(3 / angle_scale) / 3;
        ps.F[k] = (c != 0 && base_F < scaled && (int64_t)(1 / angle_scale) > 1) ? (int32_t)scaled : base_F;
        ps.actual[k] = actual, ps.corr[k] = c;
    }
}

// binmin / binmax of _binSamples (mcsamples.py:1486-1496)
static inline void bin_edges(const gd_param2d& p, double* binmin, double* binmax) {
    const double border = (p.range_max - p.range_min) * 0.1;
    double lo = np_minimum(p.param_min, p.range_min);
    if (!p.has_limits_bot) lo = lo - border;
    double hi = np_maximum(p.param_max, p.range_max);
    if (!p.has_limits_top) hi = hi + border;
    *binmin = lo, *binmax = hi;
}

// The scalar tail of _initParam (mcsamples.py:1440-1484) for one parameter, given what the quantile select and the base
// statistics delivered: q = {range_confidence quantile, its mirror, the deciles 0.1 .. 0.9}.  The same fp64 operations in
// the order MCSamples._init_params performs them (np.min over the spans of four, Python's min(err, scale)).
// `rec` arrives with has_limits_bot / has_limits_top as the prior ranges set them (_initLimits) and leaves with
// range_min, range_max, sigma_range and the limit flags final.
static inline void prepare_tail(const double q[11], double col_min, double col_max, double err, double limmin, double limmax,
                                gd_prepared_param* rec) {
    double confids[11];
    confids[0] = col_min;
    for (int k = 0; k < 9; ++k) confids[1 + k] = q[2 + k];
    confids[10] = col_max;
    double diffs[7];
    for (int k = 0; k < 7; ++k) diffs[k] = confids[k + 4] - confids[k];
    double mn = diffs[0];
    for (int k = 1; k < 7; ++k) mn = np_minimum(mn, diffs[k]);
    const double scale = mn / 1.049;
    bool flat = true;
    const double lo = err * 1.049, hi = scale * 1.5;
    for (int k = 0; k < 7; ++k) flat = flat && (diffs[k] > lo) && (diffs[k] < hi);
    rec->sigma_range = flat ? scale : (scale < err ? scale : err);  // min(par.err, scale)
    double range_min = q[0], range_max = q[1];
    const double smooth_1D = rec->sigma_range * 0.4;
    if (rec->has_limits_bot) {
        if (range_min - limmin > 2 * smooth_1D && col_min - limmin > smooth_1D)
            rec->has_limits_bot = 0;  // long way from limit
        else
            range_min = limmin;
    }
    if (rec->has_limits_top) {
        if (limmax - range_max > 2 * smooth_1D && limmax - col_max > smooth_1D)
            rec->has_limits_top = 0;
        else
            range_max = limmax;
    }
    if (!rec->has_limits_bot) range_min -= smooth_1D * 2;
    if (!rec->has_limits_top) range_max += smooth_1D * 2;
    rec->range_min = range_min, rec->range_max = range_max;
}

// Thresholds the batched call and the preparation entry (gd_prepare_params, which enqueues ahead what the call starts with)
// both read: the fewest pairs of the base grid's class that take the byte-index route, and min_corr of the N_eff estimate.
static constexpr int kByteIndexMinPairs = 64;
static constexpr double kNeffMinCorr = 0.05;
// The choreography's fixed choices (each was a tuning knob while it was measured; the figures are in DESIGN.md §1 and §8).
// Two optimiser parts: the second's DCT / fixed point beside the first's get_h and convolution.  More, smaller parts were
// measured (3 / 4 / 12: 31.2 / 32.1 / 31.4 ms per C3 step against 30.5 with two): the chip is busy either way, and a part
// below two blocks per CU leaves the fixed-point kernel's tail exposed.
static constexpr size_t kKoptParts = 2;
// The fixed-point kernel holds one pair per CU (its matrix lives in the CU's registers and LDS): parts of a whole number of
// rounds over the 256 CUs leave no extra, mostly empty round (1279 pairs as 640 + 639 are 3 + 3 rounds, as 512 + 767: 2 + 3).
static constexpr size_t kKoptPartAlign = 256;
// What the N_eff launch waits once the binning chain is being enqueued (its launches go out)
static constexpr int kNeffHoldUs = 120;
// Pairs of a call's first convolution batch / of every other one, where the settings leave them open
static constexpr int kFirstBatch = 128, kMaxBatch = 320;

// ---- effective sample numbers (chains.py:477-574 via mcsamples.py:1230-1235) -------------------------------------------
struct NeffInput {
    int64_t N;
    double norm, sum_w2;
};

// the scalar half of getEffectiveSamplesGaussianKDE given the seven batched lag sums; `lag_sum(k)` fetches another lag
static inline int neff_from_lags(const NeffInput& in, int64_t maxoff, double min_corr, const double* sums, int nseed_tail,
                                 const std::function<int(int64_t, double*)>& lag_sum, double* neff_out) {
    const int64_t N = in.N;
    if (maxoff > N / 10) maxoff = N / 10;
    const int64_t uncorr_len = N / 2;
    int64_t nav = 0;
    for (int64_t k = uncorr_len; k < uncorr_len + 5; ++k) nav += N - k;
    double s5 = 0.0;
    for (int q = 0; q < 5; ++q) s5 += sums[q];
    const double uncorr_term = s5 / (double)nav;
    const double n = (double)N;
    std::map<int64_t, double> cache;
    for (int q = 0; q < nseed_tail; ++q) cache[q + 1] = sums[5 + q];  // lags 1, 2
    int rc = 0;
    auto corr_k = [&](int64_t k) -> double {
        auto it = cache.find(k);
        double v;
        if (it == cache.end()) {
            v = NAN;
            const int e = lag_sum(k, &v);
            if (e) rc = e;
            cache[k] = v;
        } else {
            v = it->second;
        }
        return v - (n - (double)k) * uncorr_term;
    };
    const double corr0 = in.sum_w2;
    const double threshold = min_corr * corr0;
    const double c1 = corr_k(1);
    double Nn;
    if (c1 < threshold) {
        Nn = corr0;
    } else {
        const double c2 = corr_k(2);
        if (c2 > threshold) {
            int64_t max_k = maxoff;
            while (max_k > 10) {
                if (corr_k(max_k / 3) >= threshold) break;
                max_k /= 3;
            }
            const int64_t step_size = max_k < 20 ? 1 : max_k / 10;
            double cum_sum = c1 + c2;
            for (int64_t k = 3; k < maxoff + 1; k += step_size) {
                const double test_val = corr_k(k);
                if (test_val < threshold) break;
                cum_sum += k > 3 ? test_val * (double)step_size : (test_val * (double)step_size) / 2;
            }
            Nn = corr0 + 2 * cum_sum;
        } else {
            Nn = corr0 + 2 * c1;
        }
    }
    if (rc) return rc;
    *neff_out = py_pow(in.norm, 2.0) / Nn;
    return 0;
}

// The first launch of the N_eff lag sums for m columns, from their autocovariance probe (lag0: m x nl sums at lags
// 0 .. nl - 1, nl = min(8, N / 10 + 1)): the kernel width and the largest offset per column, the lag list of the launch.
// Returns -1, or the row of the first column whose correlation outlasts the probe (getCorrelationLength's long route).
struct LagPlan {
    std::vector<double> inv4s2;
    std::vector<int64_t> maxoffs, lags;
    int ntail = 0;  // 1: lag 1 rides behind the five lags from N / 2; 2: lag 2 as well
};
static inline int lag_plan(int64_t N, int m, int nl, const double* lag0, const double* var, const double* sigma_range,
                           const double* err, double min_corr, LagPlan& lp) {
    const int64_t max_off = N / 10;
    lp.inv4s2.assign(m, NAN), lp.maxoffs.assign(m, 0), lp.lags.clear(), lp.ntail = 0;
    bool all_uncorrelated_at_lag_1 = true;  // by the probe: then the speculative corr_k(2) is left out of the launch
    for (int row = 0; row < m; ++row) {
        double c[8];
        for (int k = 0; k < nl; ++k) c[k] = lag0[(size_t)row * nl + k] / (double)(N - k) / var[row];
        int first_below = -1;
        for (int k = 0; k < nl; ++k)
            if (!(c[k] > min_corr * c[0])) {
                first_below = k;
                break;
            }
        if (first_below != 1) all_uncorrelated_at_lag_1 = false;
        double corrlen;
        if (first_below >= 0) {
            double sum = 0.0;
            for (int k = 1; k < first_below; ++k) sum += c[k];
            corrlen = c[0] + 2 * sum;
        } else if (nl == max_off + 1) {
            corrlen = c[0];
        } else {
            return row;
        }
        const double sr = sigma_range[row];
        const double kstd = ((isnan(sr) || sr == 0.0) ? err[row] : sr) * 0.2;  // (par.sigma_range or self.sddev[j]) * 0.2
        lp.inv4s2[row] = 1.0 / (4 * py_pow(kstd, 2.0));
        lp.maxoffs[row] = (int64_t)(corrlen * 1.5) + 4;
    }
    const int64_t uncorr_len = N / 2;
    for (int64_t k = uncorr_len; k < uncorr_len + 5; ++k) lp.lags.push_back(k);
    // corr_k(1) always; corr_k(2) -- needed only by a chain still correlated at lag 1 (chains.py:541-545) -- rides along
    // unless the probe shows every column below the threshold at lag 1 already: six exponentials per sample instead of
    // seven (the launch is bound by them); a column the probe misjudged fetches its lag 2 by itself (neff_from_lags)
    for (int64_t k : {1, 2})
        if (k <= N / 10 && (k == 1 || !all_uncorrelated_at_lag_1)) lp.lags.push_back(k), ++lp.ntail;
    return -1;
}

// ---- the bandwidth plan (mcsamples.py:1325-1409) ----------------------------------------------------------------------
struct Plan {
    std::vector<int8_t> branch;        // 0 A, 1 B, 2 C
    std::vector<uint8_t> has_limits;   // parx.has_limits or pary.has_limits
    std::vector<double> rangex, rangey, ratio, neff, fallback_t;
    // branch A only (indexed by pair; valid where branch == 0)
    std::vector<int32_t> si, sj;       // the sheared pair's columns (swapped when y carries the limit)
    std::vector<uint8_t> swap, has_imin, has_imax;
    std::vector<double> imin, imax, S, r;  // S: 4 per pair, r: 2 per pair
};

static inline bool has_limits(const gd_param2d& p) { return p.has_limits_bot || p.has_limits_top; }

static inline int make_plan(const gd_batch2d_settings& s, const gd_param2d* par, int n, const double* cov,
                            const PairScalars& ps, const std::vector<double>& rngx, const std::vector<double>& rngy,
                            double min_corr, Plan& pl, std::string& err) {
    const int P = (int)ps.jx.size();
    pl.branch.resize(P), pl.has_limits.resize(P), pl.rangex = rngx, pl.rangey = rngy, pl.ratio.resize(P);
    pl.neff.assign(P, NAN), pl.fallback_t.assign(P, NAN);
    pl.si.assign(P, -1), pl.sj.assign(P, -1), pl.swap.assign(P, 0), pl.has_imin.assign(P, 0), pl.has_imax.assign(P, 0);
    pl.imin.assign(P, NAN), pl.imax.assign(P, NAN), pl.S.assign((size_t)4 * P, NAN), pl.r.assign((size_t)2 * P, NAN);
    for (int k = 0; k < P; ++k) {
        const gd_param2d &px = par[ps.jx[k]], &py = par[ps.jy[k]];
        const bool limx = has_limits(px), limy = has_limits(py);
        pl.has_limits[k] = limx || limy;
        const bool do_correlated = !limx || !limy;
        const double c = ps.actual[k], absc = fabs(c);
        const bool is_A = (min_corr < absc) && (absc <= s.max_corr_2D) && do_correlated;
        const bool is_B = !is_A && ((absc > s.max_corr_2D) || (!do_correlated && (c > 0.8)));
        pl.branch[k] = is_A ? 0 : (is_B ? 1 : 2);
        pl.ratio[k] = np_minimum(py.sigma_range / rngy[k], px.sigma_range / rngx[k]);
        if (!is_A) continue;
        int i = ps.jx[k], j = ps.jy[k];
        if (px.has_limits_bot) pl.has_imin[k] = 1, pl.imin[k] = px.range_min;
        if (px.has_limits_top) pl.has_imax[k] = 1, pl.imax[k] = px.range_max;
        if (limy) {
            std::swap(i, j);
            pl.swap[k] = 1;
            if (py.has_limits_bot) pl.has_imin[k] = 1, pl.imin[k] = py.range_min;
            if (py.has_limits_top) pl.has_imax[k] = 1, pl.imax[k] = py.range_max;
        }
        pl.si[k] = i, pl.sj[k] = j;
        if (!chol_shear(cov[(size_t)i * n + i], cov[(size_t)j * n + i], cov[(size_t)j * n + j], &pl.S[(size_t)4 * k],
                        &pl.r[(size_t)2 * k])) {
            err = "Matrix is not positive definite";  // numpy.linalg.LinAlgError out of np.linalg.cholesky
            return GD_ERR_BADARG;
        }
    }
    return 0;
}

// N_eff per pair (min of the two parameters', mcsamples.py:1329-1331) and the fallback time of branch C (:1396-1397)
static inline void fill_plan(const gd_param2d* par, const PairScalars& ps, Plan& pl, const double* pair_neff = nullptr) {
    const int P = (int)ps.jx.size();
    for (int k = 0; k < P; ++k) {
        // (pair_neff: the caller's own estimate per pair -- use_effective_samples_2D, mcsamples.py:1322-1328)
        pl.neff[k] = pair_neff ? pair_neff[k] : np_minimum(par[ps.jx[k]].neff, par[ps.jy[k]].neff);
        if (pl.branch[k] == 2) pl.fallback_t[k] = py_pow(pl.ratio[k] / py_pow(pl.neff[k], 1.0 / 6), 2.0);
    }
}

// ---- persistent state of a context's batched calls --------------------------------------------------------------------
struct IdxCol {
    void* ptr = nullptr;
    double binmin = NAN, width = NAN;
    bool valid = false;
};

struct Pending {  // a call whose result copies may still be in flight
    std::vector<void*> blocks;
    int32_t tok_main = -1, tok_twin = -1;
    void* twin = nullptr;
    bool live = false;
};

struct State {
    std::mutex mu;
    std::vector<std::pair<void*, int64_t>> free_blocks;  // (device pointer, capacity)
    std::map<void*, int64_t> capacity;                   // of every block handed out
    int64_t cached_bytes = 0;
    std::map<std::tuple<int, int, int>, IdxCol> idx;     // (column, F, kind): read and written through IndexCache only
    Pending prev;                                        // the last lazily delivered call
    void* aux = nullptr;                                 // third context (stream) of large calls: shear chain, get_h
    void* aux2 = nullptr;                                // fourth: the DEFERRED shear chain + up-scaled classes
    // work the preparation entry (gd_prepare_params) enqueued ahead of the next batched call: the binding's own record
    // (batch2d.hip), and whether N_eff lag sums are among it (neff_batch then has nothing to hold back)
    void* ahead = nullptr;
    std::atomic<bool> neff_ahead{false};
    int64_t exchanges_entered = 0;                       // N_eff collectives the library ENTERED over the communicator (whether or
                                                         // not the call went on to succeed): gd_batch2d_exchanges
    static constexpr int64_t kCacheLimit = 16LL << 30;
};

struct Pool {
    State& st;
    const Ops& ops;
    void* h;
    void* take(int64_t bytes, int* rc) {
        {
            std::lock_guard<std::mutex> g(st.mu);
            int best = -1;
            for (size_t k = 0; k < st.free_blocks.size(); ++k) {
                const int64_t cap = st.free_blocks[k].second;
                if (cap >= bytes && cap <= 2 * bytes + (1 << 20) && (best < 0 || cap < st.free_blocks[best].second)) best = (int)k;
            }
            if (best >= 0) {
                void* p = st.free_blocks[best].first;
                st.cached_bytes -= st.free_blocks[best].second;
                st.free_blocks.erase(st.free_blocks.begin() + best);
                return p;
            }
        }
        void* p = nullptr;
        int e = ops.dev_alloc(h, bytes, &p);
        if (e == GD_ERR_NOMEM) {  // hand the cached blocks back and retry once
            drop_cached();
            e = ops.dev_alloc(h, bytes, &p);
        }
        if (e) {
            *rc = e;
            return nullptr;
        }
        std::lock_guard<std::mutex> g(st.mu);
        st.capacity[p] = bytes;
        return p;
    }
    void give(void* p) {
        if (!p) return;
        std::unique_lock<std::mutex> g(st.mu);
        const int64_t cap = st.capacity[p];
        if (st.cached_bytes + cap > State::kCacheLimit) {
            st.capacity.erase(p);
            g.unlock();
            ops.dev_free(h, p);
            return;
        }
        st.free_blocks.emplace_back(p, cap);
        st.cached_bytes += cap;
    }
    void drop_cached() {
        std::vector<std::pair<void*, int64_t>> blocks;
        {
            std::lock_guard<std::mutex> g(st.mu);
            blocks.swap(st.free_blocks);
            st.cached_bytes = 0;
            for (auto& b : blocks) st.capacity.erase(b.first);
        }
        for (auto& b : blocks) ops.dev_free(h, b.first);
    }
    // a block that goes back to the pool when the scope ends, unless somebody has taken it over by then
    struct Lease {
        Pool& pool;
        void* p;
        ~Lease() { pool.give(p); }
        void* keep() { return std::exchange(p, nullptr); }
    };
};

// The index columns of the resident samples, cached per (column, grid size, kind) with the edges they were binned with.
// A column's block is published as the column's own -- not yet valid -- BEFORE any launch writes it, and becomes valid when
// the launch has been committed: a launch that fails leaks nothing and leaves nothing valid behind.
struct IndexCache {
    enum Kind { kBytes = 1, kU16 = 2 };  // (also the bytes per sample)
    State& st;
    struct Stale {
        std::vector<int32_t> cols;
        std::vector<double> binmin, width;
        std::vector<void*> bufs;
    };
    // the columns of `cols` (edges binmin / width, parallel to it) that are not cached with these edges, each with its block
    // of N samples (from `pool` where it has none); 0, or the code of the allocation that failed
    int stale(Pool& pool, const std::vector<int32_t>& cols, int F, Kind kind, int64_t N, const double* binmin, const double* width,
              Stale& out) {
        for (size_t q = 0; q < cols.size(); ++q) {
            const auto key = std::make_tuple((int)cols[q], F, (int)kind);
            IdxCol c;
            {
                std::lock_guard<std::mutex> g(st.mu);
                c = st.idx[key];
            }
            if (c.valid && c.binmin == binmin[q] && c.width == width[q]) continue;
            if (!c.ptr) {
                int rc = 0;
                c.ptr = pool.take(N * (int)kind + 64, &rc);
                if (!c.ptr) return rc;
            }
            {
                std::lock_guard<std::mutex> g(st.mu);
                IdxCol& e = st.idx[key];
                e.ptr = c.ptr, e.valid = false;
            }
            out.cols.push_back(cols[q]), out.binmin.push_back(binmin[q]), out.width.push_back(width[q]), out.bufs.push_back(c.ptr);
        }
        return 0;
    }
    // after the launch that wrote them: the edges, and valid -- on the byte route (`bad`: samples outside the grid per
    // column) only a column that holds every sample
    void commit(const Stale& done, int F, Kind kind, const int64_t* bad = nullptr) {
        std::lock_guard<std::mutex> g(st.mu);
        for (size_t q = 0; q < done.cols.size(); ++q) {
            IdxCol& c = st.idx[std::make_tuple((int)done.cols[q], F, (int)kind)];
            c.binmin = done.binmin[q], c.width = done.width[q], c.valid = !bad || bad[q] == 0;
        }
    }
    void* lookup(int col, int F, Kind kind) {
        std::lock_guard<std::mutex> g(st.mu);
        auto it = st.idx.find(std::make_tuple(col, F, (int)kind));
        return it == st.idx.end() ? nullptr : it->second.ptr;
    }
    // a column found bad after it was committed (work enqueued ahead): stale, if `ptr` is still its block
    void mark_stale(int col, int F, Kind kind, const void* ptr) {
        std::lock_guard<std::mutex> g(st.mu);
        auto it = st.idx.find(std::make_tuple(col, F, (int)kind));
        if (it != st.idx.end() && it->second.ptr == ptr) it->second.valid = false;
    }
    void invalidate() {  // the samples changed: every column keeps its block and is binned again
        std::lock_guard<std::mutex> g(st.mu);
        for (auto& kv : st.idx) kv.second.valid = false;
    }
    void release() {  // every block back to the pool
        std::lock_guard<std::mutex> g(st.mu);
        for (auto& kv : st.idx)
            if (kv.second.ptr) st.free_blocks.emplace_back(kv.second.ptr, st.capacity[kv.second.ptr]);
        st.idx.clear();
    }
};

static inline int complete_pending(State& st, const Ops& ops, void* h, Pending& pd) {
    if (!pd.live) return 0;
    int rc = 0;
    if (pd.tok_main >= 0) rc = ops.copy_wait(h, pd.tok_main);
    if (!rc && pd.twin && pd.tok_twin >= 0) rc = ops.copy_wait(pd.twin, pd.tok_twin);
    Pool pool{st, ops, h};
    for (void* p : pd.blocks) pool.give(p);
    pd.blocks.clear();
    pd.live = false;
    return rc;
}

static inline int finish_all(State& st, const Ops& ops, void* h) { return complete_pending(st, ops, h, st.prev); }

static inline void invalidate_index_columns(State& st) { IndexCache{st}.invalidate(); }

// frees every device block the state holds (context teardown / new sample set)
static inline void release_all(State& st, const Ops& ops, void* h) {
    finish_all(st, ops, h);
    Pool pool{st, ops, h};
    IndexCache{st}.release();
    pool.drop_cached();
    if (st.aux) {  // (attached to the sample set that is going away)
        ops.destroy_aux(st.aux);
        st.aux = nullptr;
    }
    if (st.aux2) {
        ops.destroy_aux(st.aux2);
        st.aux2 = nullptr;
    }
}

// ---- hand-offs between the threads of a call --------------------------------------------------------------------------
// Every wait of the choreography is a sleeping poll: the quanta and bounds were tuned with the wake-up latency on the
// critical path.  quantum_us 0: yield instead of sleeping; bound_us 0: until ready.  False: the bound passed.
template <class Ready>
static inline bool poll_until(const Ready& ready, int quantum_us, int64_t bound_us) {
    const auto t0 = std::chrono::steady_clock::now();
    while (!ready()) {
        if (bound_us > 0 && std::chrono::steady_clock::now() - t0 >= std::chrono::microseconds(bound_us)) return false;
        quantum_us > 0 ? std::this_thread::sleep_for(std::chrono::microseconds(quantum_us)) : std::this_thread::yield();
    }
    return true;
}

// One thread tells others that something exists.  A gate opens once, with a code (0: what the consumer waits for is
// there), and stays open.  Its producer holds an Opener: when the producer's scope ends -- return, early return or
// exception -- a gate that is still closed opens with the code the producer left (GD_ERR_HIP if none).  A wait without a
// bound is served only on a gate that has an Opener, which therefore has to exist before the consumer can start waiting
// (start() makes it in the thread that starts the producer); on any other gate such a wait fails at once instead of hanging.
class Gate {
    static constexpr int kClosed = INT_MIN;
    std::atomic<int> state_{kClosed};
    std::atomic<bool> held_{false};

public:
    void open(int code = 0) {
        int closed = kClosed;
        state_.compare_exchange_strong(closed, code, std::memory_order_release, std::memory_order_relaxed);
    }
    bool is_open() const { return state_.load(std::memory_order_acquire) != kClosed; }
    int code() const { return state_.load(std::memory_order_acquire); }  // of an open gate
    // true: the gate is open (code() is what the producer left)
    bool wait(int quantum_us, int64_t bound_us) const {
        if (bound_us <= 0 && !held_.load() && !is_open()) return false;
        return poll_until([this] { return is_open(); }, quantum_us, bound_us);
    }
    class Opener {
        Gate* gate_;
        int code_ = GD_ERR_HIP;

    public:
        explicit Opener(Gate* g = nullptr) : gate_(g) {
            if (g) g->held_.store(true);
        }
        Opener(Opener&& o) noexcept : gate_(o.gate_), code_(o.code_) { o.gate_ = nullptr; }
        void leave(int code) { code_ = code; }  // what the gate opens with if nobody has opened it when the scope ends
        ~Opener() {
            if (gate_) gate_->open(code_);
        }
    };
};

// A thread of the call and the one place its result is read: whoever needs it first waits for the thread, everyone
// after that gets the same code.
struct Worker {
    std::future<int> result;
    std::mutex mu;
    int rc = 0;
    int join(bool* was_running = nullptr) {
        std::lock_guard<std::mutex> g(mu);
        if (was_running) *was_running = result.valid();
        if (result.valid()) rc = result.get();
        return rc;
    }
};

template <class F>
struct AtExit {  // f runs when the scope ends, however it ends
    F f;
    ~AtExit() { f(); }
};
template <class F>
AtExit(F) -> AtExit<F>;

// ---- the optimiser's launches ------------------------------------------------------------------------------------------
struct Launch {
    int F = 0;
    std::vector<int> ks;   // plan indices in batch order
    int na = 0;            // leading sheared rows
    void* d_hist = nullptr;  // class buffer (the sheared histograms when the launch holds nothing else)
    std::vector<int> pos;  // positions within the class buffer of the non-sheared rows
    bool whole = false;    // the buffer as it lies
    // staged mode
    void* d_batch = nullptr;
    bool own = false;
    void* d_rows = nullptr;
    int32_t ticket = -1;
    std::vector<double> ne, fb, ci;
    std::vector<int32_t> dc;
};

// the size of a part of the base grid's optimiser launches (total = its own pairs + the sheared pairs)
static inline size_t base_part_size(size_t total, int F, int split_min) {
    size_t part = std::max<size_t>((size_t)split_min, (total + kKoptParts - 1) / kKoptParts);
    if (F == 256 && part > kKoptPartAlign) part = std::max(kKoptPartAlign, (part + kKoptPartAlign / 2 - 1) / kKoptPartAlign * kKoptPartAlign);
    return part;
}

// The optimiser's launches of a call, from the plan alone (no device call; d_hist is the caller's to fill): one launch per
// grid-size class that has optimiser pairs (branch C), in class order; `staged` cuts the base grid's launch into parts.  The
// sheared pairs (branch A) lead one launch of the base class -- the first, or with the deferred chain the last, which then
// takes whatever is left -- or make a launch of their own when the base class has no optimiser pairs.
static inline std::vector<Launch> plan_launches(const std::vector<int8_t>& branch, const std::vector<int>& F_list,
                                                const std::map<int, std::vector<int>>& classes, int base_F, bool staged,
                                                bool shear_deferred, int split_min) {
    std::vector<int> A;
    for (int k = 0; k < (int)branch.size(); ++k)
        if (branch[k] == 0) A.push_back(k);
    const int nA = (int)A.size();
    std::vector<Launch> launches;
    bool merged = false;
    for (int F : F_list) {
        const std::vector<int>& mem = classes.at(F);
        std::vector<int> pos_C;
        for (int q = 0; q < (int)mem.size(); ++q)
            if (branch[mem[q]] == 2) pos_C.push_back(q);
        if (pos_C.empty()) continue;
        const bool base = F == base_F;  // (any other class: one launch of its own pairs)
        const size_t total = pos_C.size() + (base ? (size_t)nA : 0);
        const size_t part = (base && staged && (int)pos_C.size() >= split_min) ? base_part_size(total, F, split_min) : total;
        const size_t nparts = std::max<size_t>(1, (total + part - 1) / part);
        for (size_t c0 = 0, ip = 0; c0 < pos_C.size(); ++ip) {
            Launch L;
            const bool carries = shear_deferred ? (ip + 1 == nparts || pos_C.size() - c0 <= part) : ip == 0;
            L.F = F, L.na = (base && carries) ? nA : 0;
            size_t take = std::min(pos_C.size() - c0, part > (size_t)L.na ? part - (size_t)L.na : (size_t)1);
            if (shear_deferred && carries) take = pos_C.size() - c0;
            L.pos.assign(pos_C.begin() + c0, pos_C.begin() + c0 + take);
            c0 += take;
            L.whole = L.na == 0 && L.pos.size() == mem.size();
            for (int q = 0; q < L.na; ++q) L.ks.push_back(A[q]);
            for (int q : L.pos) L.ks.push_back(mem[q]);
            launches.push_back(std::move(L));
        }
        merged = merged || base;
    }
    if (nA && !merged) {
        Launch L;
        L.F = base_F, L.na = nA, L.whole = true, L.ks = A;
        launches.push_back(std::move(L));
    }
    return launches;
}

// ---- the call ----------------------------------------------------------------------------------------------------------
// The environment switches of a call, read once when the call is made (tests set them between calls of one process).
struct Switches {
    bool log = getenv("GDHIP_BATCH_LOG") != nullptr;  // the host timeline on stderr when the call returns
    // the reference paths of the tests: the chain joined in front of the optimiser (=0) / its threshold in pairs / one binning launch
    bool shear_deferred = !getenv("GDHIP_BATCH_SHEAR_DEFERRED") || atoi(getenv("GDHIP_BATCH_SHEAR_DEFERRED")) != 0;
    int shear_deferred_min = getenv("GDHIP_BATCH_SHEAR_DEFERRED_MIN") ? atoi(getenv("GDHIP_BATCH_SHEAR_DEFERRED_MIN")) : 256;
    bool one_binning = getenv("GDHIP_BATCH_ONE_BINNING") != nullptr;
    // test hook: a slow second half of the chain
    int side_binning_delay_ms = getenv("GDHIP_BATCH_TEST_SIDE_BINNING_DELAY_MS") ? atoi(getenv("GDHIP_BATCH_TEST_SIDE_BINNING_DELAY_MS")) : 0;
    bool no_wsort = getenv("GDHIP_NO_WSORT") != nullptr;  // real weights: no byte-index route
};

struct Call {
    State& st;
    const Ops& ops;
    void* h;     // main context: first stream
    void* twin;  // second stream (may be null)
    const gd_batch2d_settings& s;
    gd_param2d* par;
    int n;
    const double* corrmat;
    const double* cov;
    const double* lag_probe;
    const int32_t* pairs;
    int P;
    gd_neff_exchange_fn exchange;
    void* exchange_user;
    double* grids;
    int64_t grids_doubles;
    int32_t* status_pinned;
    double* meta;
    double* levels;
    int32_t* level_status;
    std::string err;

    Call(State& st_, const Ops& ops_, void* h_, void* twin_, const gd_batch2d_settings& s_, gd_param2d* par_, int n_,
         const double* corr_, const double* cov_, const double* lag_probe_, const int32_t* pairs_, int P_,
         gd_neff_exchange_fn ex_, void* ex_user_, double* grids_, int64_t grids_doubles_, int32_t* status_, double* meta_,
         double* levels_, int32_t* level_status_)
        : st(st_), ops(ops_), h(h_), twin(twin_), s(s_), par(par_), n(n_), corrmat(corr_), cov(cov_), lag_probe(lag_probe_),
          pairs(pairs_), P(P_), exchange(ex_), exchange_user(ex_user_), grids(grids_), grids_doubles(grids_doubles_),
          status_pinned(status_), meta(meta_), levels(levels_), level_status(level_status_), pool{st_, ops_, h_}, cache{st_} {}
    // (an exception on the calling thread: no thread of the call outlives what it works on)
    ~Call() {
        conv.first_enqueued.open();
        (void)neff.join(), (void)bin.thread.join(), (void)shear.thread.join();
    }

    const Switches env;
    int64_t N = 0;
    bool unit_weights = true;
    bool byte_index_weights = false;  // real weights: the byte-index route is served too (gd_hist2d_prebinned8's sorted form)
    Pool pool;
    IndexCache cache;
    PairScalars ps;
    std::vector<int> used;
    std::vector<double> bmin, bmax;  // per column
    std::vector<double> fwx, fwy;    // per pair
    std::vector<int> F_list;         // grid sizes in order of first appearance
    std::map<int, std::vector<int>> classes;  // F -> pair indices, ascending
    std::map<int, void*> hists;               // F -> device histograms of the class, in member order (under enq_mu)
    std::mutex enq_mu;
    Plan plan;
    std::vector<double> rx, ry, cc, smooth, W;  // per pair; W: P x 3
    std::vector<int64_t> winw;
    std::vector<int32_t> flags, group;
    void* aux = nullptr;  // third context (large calls)
    Worker neff;          // the N_eff thread of a large call

    // Main binning, on the second context beside the N_eff kernels.
    struct Binning {
        Worker thread;
        // The N_eff launch (2000 resident blocks for ~3 ms: whatever is enqueued behind it on another stream waits for a wave
        // slot) holds back until the binning thread is enqueuing its chain: the binning is on the critical path, the N_eff
        // values are needed after it (a race the binning used to win by ~0.2 ms).
        Gate launching;
        bool hold_neff = false;
        // Two launches (single-triangle latency): the members of the base grid's class are put in the order the optimiser
        // takes them (its own pairs first, the sheared and rule-of-thumb pairs behind), rows [0, first_rows) -- the FIRST
        // optimiser part's -- are binned by the fused prebin + histogram call, the other rows by a second histogram launch
        // behind it, and stage A of the first part starts when the first launch has run instead of waiting for both.
        // Everything else (the later parts, every convolution, the deferred chain) joins the whole binning.  A pair's histogram
        // does not depend on its row or on the launch that fills it: results unchanged bit for bit.  first_rows 0: one launch.
        int first_rows = 0;
        Gate first_run;  // the first launch has run (or the thread has ended)
        Gate done;       // the thread has ended: the whole main binning has run
        std::vector<void*> stale;  // a class buffer whose second launch failed (under enq_mu; freed with the call's blocks)
    } bin;

    // Branch A's chain -- min/max of the sheared coordinate, re-binning of the fp64 samples -- and the up-scaled grid classes
    // behind it, on the third context.  Deferred (single-triangle latency): the first result copies can leave once the FIRST
    // optimiser part's pairs are convolved, and 642 MB of grids then take ~13 ms of PCIe, so what that first part waits for
    // decides when a triangle is delivered.  The chain then runs on a context of its own, its pairs ride in the LAST base
    // part, and the staging thread waits for it only when it builds the first launch that needs it.  Results are unchanged
    // bit for bit (a pair's grid does not depend on the part it is computed in).
    struct Shear {
        void* d_rot = nullptr;
        std::vector<int> A;
        std::vector<double> r1s, r2s;
        bool have = false;
        Worker thread;
        bool deferred = false;
        bool running = false;  // a deferred chain that the optimiser's launches may have to wait for
        // The chain's two halves are awaited separately: a launch that carries sheared rows needs the SHEARED HISTOGRAMS only,
        // not the up-scaled classes binned behind them -- the last base part's stage A used to start 2.5 ms later than its rows
        // existed (stream timeline of a C3 step: sheared histograms done at 16.9 ms, the up-scaled classes at 19.4, the last
        // part's first kernel at 19.6).  Opens with the code of shear_histograms.
        Gate hists;
    } shear;

    // Convolution and result copies.
    struct Conv {
        int64_t grid_off = 0;
        int status_at = 0;
        int batch_no = 0;
        std::vector<void*> ctxs;
        std::vector<int> side_classes;
        std::vector<int> order;           // grid sizes, largest class (in bytes) first
        std::vector<void*> call_blocks;   // everything to release once the copies have landed
        // The deferred chain starts only when the FIRST optimiser part's convolution has been enqueued (its stage A, get_h and
        // first batches get the machine ahead of the chain's 1024-thread blocks; the chain then runs beside the later parts):
        // same-box A/B, delivered triangle: chain at once 29.4-29.9 ms, released on the first part's bandwidths 28.8-29.5, on
        // its convolution 28.1-28.9; the stream of triangles 21.7 -> 21.9.  Open at once when the first launch itself needs
        // the chain, when nothing is staged, and on every error path.
        Gate first_enqueued;
        // ... and, for a single delivered call, only when that convolution has RUN: the chain's blocks take every CU for ~3 ms,
        // and started on the enqueue they ran beside the first part's convolution -- the triangle's first grids, which the 13 ms
        // of result copies wait for (a timed hold of 1000 / 2000 / 3000 / 4500 us: delivered 26.1 / 24.6 / 24.5 / 24.3 ms, stream
        // 20.4 / 20.6 / 21.6 / 22.2 against 26.5 / 19.9 without).  The signal is the status word of the first report's last batch:
        // enqueue_batch pre-sets a batch's words to kStatusPending, the batch's last launch (a copy kernel into page-locked memory)
        // overwrites them.  A STREAM of calls (settings.results_in_flight) is released on the enqueue: this call's first grids
        // queue behind the previous call's copies, and the chain beside the first convolution is the better use of the machine
        // (19.9 against 21.0 ms per triangle).
        std::atomic<const volatile int32_t*> first_run_word{nullptr};
        int reports_enqueued = 0;  // (enqueuing thread only)
    } conv;
    static constexpr int32_t kStatusPending = 0x7fffffff;

    // Host-side timeline of the call (GDHIP_BATCH_LOG=1 prints it to stderr when the call returns).
    struct Timeline {
        std::mutex mu;
        std::vector<std::pair<double, std::string>> events;
    } tl;
    static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void mark(const char* what, int a = -1, int b = -1) {
        if (!env.log) return;
        char buf[160];
        if (a >= 0 && b >= 0)
            snprintf(buf, sizeof buf, "%s (%d, %d)", what, a, b);
        else if (a >= 0)
            snprintf(buf, sizeof buf, "%s (%d)", what, a);
        else
            snprintf(buf, sizeof buf, "%s", what);
        std::lock_guard<std::mutex> g(tl.mu);
        tl.events.emplace_back(now_ms(), buf);
    }
    void dump_timeline() {
        if (!env.log || tl.events.empty()) return;
        std::sort(tl.events.begin(), tl.events.end());
        fprintf(stderr, "---- gd_density2d_batch host timeline (ms)\n");
        for (auto& e : tl.events) fprintf(stderr, "%9.3f  %s\n", e.first - tl.events[0].first, e.second.c_str());
    }

    std::mutex err_mu;
    int fail(int code, const std::string& msg) {
        std::lock_guard<std::mutex> g(err_mu);
        if (err.empty()) err = msg;
        return code;
    }
    int dev_fail(int code, void* ctx) {
        const char* m = ops.last_error(ctx);
        return fail(code, m && *m ? m : "device call failed");
    }
#define GDB_DEV(ctx_, call_)                       \
    do {                                           \
        const int rc__ = (call_);                  \
        if (rc__) return dev_fail(rc__, (ctx_));   \
    } while (0)
#define GDB_TRY(call_)            \
    do {                          \
        const int rc__ = (call_); \
        if (rc__) return rc__;    \
    } while (0)

    // -- threads.  An exception that escapes a piece of the call's work becomes the call's error and a return code ...
    template <class Fn>
    int guarded(const Fn& work) {
        try {
            return work();
        } catch (const std::exception& e) {
            return fail(GD_ERR_NOMEM, e.what());
        }
    }
    // ... and every thread of the call runs through here: bound to its context, its result always a code, and the gates it
    // produces (held from this moment, in the starting thread) open with that code when it ends, however it ends.
    std::future<int> start(void* ctx, std::function<int()> body, Gate* g1 = nullptr, Gate* g2 = nullptr) {
        return std::async(std::launch::async, [this, ctx, body = std::move(body), o1 = Gate::Opener(g1), o2 = Gate::Opener(g2)]() mutable {
            Gate::Opener a(std::move(o1)), b(std::move(o2));
            const int rc = guarded([&] { return ops.bind_thread(ctx), body(); });
            a.leave(rc), b.leave(rc);
            return rc;
        });
    }
    int join(Worker& w, const char* what) {
        bool was_running = false;
        const int e = w.join(&was_running);
        if (was_running) mark(what);
        return e;
    }
    int join_binning() { return join(bin.thread, "binning: joined"); }
    // release: the caller is not going to enqueue a first part the chain could wait for (error paths, a call whose only
    // launch needs the chain).  The staging thread's ordinary join does NOT release: by then the first part is enqueued.
    int join_shear(bool release = false) {
        if (release) conv.first_enqueued.open();
        return join(shear.thread, "shear: joined");
    }

    double* M(int k) { return meta + (size_t)k * GD_BATCH2D_META; }

    // -- N_eff of the listed columns that have none yet (the batched form of _get1DNeff, mcsamples.py:1230-1235)
    int neff_batch(const std::vector<int>& js, bool owned_only, double min_corr = kNeffMinCorr) {
        std::vector<int32_t> todo;
        for (int j : js)
            if (isnan(par[j].neff) && (!owned_only || (par[j].owned & 1))) todo.push_back(j);
        if (todo.empty()) return 0;
        mark("neff: start", (int)todo.size());
        if (s.uncorrelated_sampler) {
            for (int j : todo) par[j].neff = py_pow(s.norm, 2.0) / s.sum_w2;
            return 0;
        }
        const int m = (int)todo.size();
        const int64_t max_off = N / 10;
        const int nl = (int)std::min<int64_t>(8, max_off + 1);
        std::vector<double> lag0((size_t)m * nl);
        bool have = lag_probe != nullptr && nl == 8;
        if (have)
            for (int row = 0; row < m && have; ++row)
                for (int k = 0; k < nl; ++k) {
                    lag0[(size_t)row * nl + k] = lag_probe[(size_t)todo[row] * 8 + k];
                    if (isnan(lag0[(size_t)row * nl + k])) have = false;
                }
        if (!have) {
            std::vector<double> means(m);
            for (int row = 0; row < m; ++row) means[row] = par[todo[row]].mean;
            GDB_DEV(h, ops.autocov_lags_batch(h, todo.data(), m, means.data(), 0, nl, lag0.data()));
        }
        LagPlan lp;
        {
            std::vector<double> var(m), sr(m), er(m);
            for (int row = 0; row < m; ++row) {
                const gd_param2d& p = par[todo[row]];
                var[row] = p.var, sr[row] = p.sigma_range, er[row] = p.err;
            }
            const int long_row = lag_plan(N, m, nl, lag0.data(), var.data(), sr.data(), er.data(), min_corr, lp);
            if (long_row >= 0) {
                char buf[160];
                snprintf(buf, sizeof buf, "column %d: the chain's correlation outlasts the 8-lag probe (getCorrelationLength's long route)",
                         (int)todo[long_row]);
                return fail(GD_BATCH2D_NEED_NEFF, buf);
            }
        }
        const int L = (int)lp.lags.size();
        std::vector<double> sums((size_t)m * L);
        mark("neff: probe done");
        // (lag sums the preparation entry has already enqueued for this sample set: nothing to hold back, the binding of
        // kde_lag_sums_batch hands their result over or, on any mismatch, waits for them and launches afresh)
        if (bin.hold_neff && !st.neff_ahead.load()) {
            if (bin.launching.wait(0, 2000)) std::this_thread::sleep_for(std::chrono::microseconds(kNeffHoldUs));
            mark("neff: binning chain enqueued");
        }
        GDB_DEV(h, ops.kde_lag_sums_batch(h, todo.data(), m, lp.inv4s2.data(), lp.lags.data(), L, sums.data()));
        mark("neff: lag sums done");
        const NeffInput in{N, s.norm, s.sum_w2};
        for (int row = 0; row < m; ++row) {
            const int col = todo[row];
            const double i4 = lp.inv4s2[row];
            auto lag_sum = [&](int64_t k, double* out) -> int { return ops.kde_lag_sums(h, col, i4, &k, 1, out); };
            double v = NAN;
            const int e = neff_from_lags(in, lp.maxoffs[row], min_corr, &sums[(size_t)row * L], lp.ntail, lag_sum, &v);
            if (e) return dev_fail(e, h);
            par[col].neff = v;
        }
        return 0;
    }

    // -- multi-rank: the other ranks' N_eff values, then whatever nobody owned (mcsamples._neff_complete)
    int neff_exchange(bool* exchanged) {
        if (exchange && !*exchanged) {
            *exchanged = true;
            std::vector<double> v(n);
            for (int j = 0; j < n; ++j) v[j] = par[j].neff;
            if (exchange(exchange_user, v.data(), n)) return fail(GD_ERR_HIP, "N_eff exchange failed");
            for (int j = 0; j < n; ++j)
                if (isnan(par[j].neff)) par[j].neff = v[j];
        } else if (!exchange && s.comm_exchange && !*exchanged) {
            // the library's own exchange: every parameter is owned by exactly one rank, so a sum all-reduce of the owners'
            // values (zero elsewhere) delivers all of them; one collective per call on every rank, whatever its share needs
            *exchanged = true;
            if (!ops.comm_world || ops.comm_world(h) < 1) return fail(GD_ERR_BADARG, "comm_exchange without a communicator (gd_comm_init)");
            {  // counted BEFORE the collective is issued: a caller whose call fails later must know that this rank took part
                std::lock_guard<std::mutex> g(st.mu);
                ++st.exchanges_entered;
            }
            std::vector<double> v(n, 0.0);
            for (int j = 0; j < n; ++j)
                if ((par[j].owned & 1) && !isnan(par[j].neff)) v[j] = par[j].neff;
            GDB_DEV(h, ops.comm_allreduce_sum(h, v.data(), n));
            for (int j = 0; j < n; ++j)
                if (isnan(par[j].neff) && v[j] > 0) par[j].neff = v[j];
        }
        return 0;
    }
    int neff_complete(bool* exchanged) {
        const int rc = neff_exchange(exchanged);
        if (rc || s.pair_neff) return rc;  // (per-pair values from the caller: no parameter's own N_eff is needed)
        return neff_batch(used, false);
    }

    // -- index columns: the stale ones among `cols` for grid size F, with this call's edges
    int stale_columns(const std::vector<int32_t>& cols, int F, IndexCache::Kind kind, IndexCache::Stale& todo) {
        std::vector<double> b0, w;
        for (int j : cols) b0.push_back(bmin[j]), w.push_back((bmax[j] - bmin[j]) / (F - 1));
        const int rc = cache.stale(pool, cols, F, kind, N, b0.data(), w.data(), todo);
        return rc ? dev_fail(rc, h) : 0;
    }
    // the columns of a class's pairs in order of first appearance: every x then every y, or pair by pair
    std::vector<int32_t> class_columns(const std::vector<int>& members, bool x_then_y) const {
        std::vector<int32_t> cols;
        std::vector<char> seen(n, 0);
        auto add = [&](int j) {
            if (!seen[j]) seen[j] = 1, cols.push_back(j);
        };
        for (int k : members) {
            add(ps.jx[k]);
            if (!x_then_y) add(ps.jy[k]);
        }
        if (x_then_y)
            for (int k : members) add(ps.jy[k]);
        return cols;
    }
    // the u16 index columns of a grid-size class: the stale ones in ONE launch where the library has it (the up-scaled
    // classes used to cost a launch per column -- 12 launches of 20-70 us between the shear chain and their histograms),
    // a single one and whatever is left by the single-column entry
    int index_columns16(void* ctx, const std::vector<int32_t>& cols, int F) {
        IndexCache::Stale todo;
        if (ops.prebin_batch) GDB_TRY(stale_columns(cols, F, IndexCache::kU16, todo));
        if (todo.cols.size() < 2) return 0;
        GDB_DEV(ctx, ops.prebin_batch(ctx, todo.cols.data(), (int)todo.cols.size(), todo.binmin.data(), todo.width.data(), F, todo.bufs.data()));
        cache.commit(todo, F, IndexCache::kU16);
        return 0;
    }
    int index_column16(void* ctx, int j, int F, void** out) {
        IndexCache::Stale todo;
        GDB_TRY(stale_columns({j}, F, IndexCache::kU16, todo));
        if (!todo.cols.empty()) {
            GDB_DEV(ctx, ops.prebin(ctx, j, todo.binmin[0], todo.width[0], F, todo.bufs[0]));
            cache.commit(todo, F, IndexCache::kU16);
        }
        *out = cache.lookup(j, F, IndexCache::kU16);
        return 0;
    }

    // -- prebin + batched 2D histograms of every grid-size class on context `ctx` (mcsamples.py:1486-1498, 1724-1728)
    // part 0: every grid-size class; 1: the class with the most pairs only; 2: the others.  Large calls bin the main class
    // on the second stream and the few pairs of the up-scaled classes behind the shear chain on the third: they used to
    // follow the main class on the second stream -- 1.4 ms of small launches between the end of the O(N) phase and the
    // first optimiser kernel, with the other two streams idle.
    int main_class() const {
        int best = F_list.empty() ? 0 : F_list[0];
        for (int F : F_list)
            if (classes.at(F).size() > classes.at(best).size()) best = F;
        return best;
    }
    void publish_hists(int F, void* d) {
        std::lock_guard<std::mutex> g(enq_mu);
        hists[F] = d;
    }
    int binning(void* ctx, int part = 0) {
        const int main_F = main_class();
        for (int F : F_list) {
            if ((part == 1 && F != main_F) || (part == 2 && F == main_F)) continue;
            const std::vector<int>& members = classes.at(F);
            const int B = (int)members.size();
            int rc = 0;
            if (F == 256 && (unit_weights || byte_index_weights) && B >= kByteIndexMinPairs) {
                // the base grid of a unit-weight triangle: byte indices, packed 16-bit counters, one block per pair;
                // the stale byte index columns and the histograms over them go out back to back: one wait for both
                IndexCache::Stale todo;
                GDB_TRY(stale_columns(class_columns(members, true), 256, IndexCache::kBytes, todo));
                std::vector<const void*> ix(B), iy(B);
                for (int q = 0; q < B; ++q) {
                    ix[q] = cache.lookup(ps.jx[members[q]], 256, IndexCache::kBytes);
                    iy[q] = cache.lookup(ps.jy[members[q]], 256, IndexCache::kBytes);
                }
                Pool::Lease d{pool, pool.take((int64_t)B * 65536 * 8, &rc)};
                if (!d.p) return dev_fail(rc, h);
                const int ntodo = (int)todo.cols.size();
                std::vector<int64_t> bad(ntodo + 1, 0);
                mark("binning: prebin8 + hist2d launch", ntodo, B);
                bin.launching.open();
                // (two launches: the first optimiser part's rows, then the others -- see Binning)
                const int B1 = (F == main_F && bin.first_rows > 0 && bin.first_rows < B) ? bin.first_rows : B;
                int e = ops.prebin8_hist2d(ctx, todo.cols.data(), ntodo, todo.binmin.data(), todo.width.data(), todo.bufs.data(),
                                           bad.data(), B1, ix.data(), iy.data(), d.p);
                mark("binning: prebin8 + hist2d done", B1);
                if (e == 0 || e == GD_ERR_SOLVER) cache.commit(todo, 256, IndexCache::kBytes, bad.data());
                if (e == 0) {
                    void* rows = d.keep();  // the class's buffer from here on
                    publish_hists(F, rows);
                    if (B1 == B) continue;
                    bin.first_run.open();
                    e = ops.hist2d_prebinned8(ctx, B - B1, ix.data() + B1, iy.data() + B1, (char*)rows + (int64_t)B1 * 65536 * 8);
                    mark("binning: the other rows done", B - B1);
                    if (e == 0) continue;
                    // the first part may be reading its rows: the block lives until the call ends
                    std::lock_guard<std::mutex> g(enq_mu);
                    hists.erase(F);
                    bin.stale.push_back(rows);
                }
                if (e != GD_ERR_SOLVER) return dev_fail(e, ctx);  // (else: the u16 / u32 path below redoes the class)
            }
            bin.launching.open();  // (this class enqueues as it goes)
            GDB_TRY(index_columns16(ctx, class_columns(members, false), F));
            std::vector<const void*> ix(B), iy(B);
            for (int y = 0; y < 2; ++y)  // (every x column, then every y column)
                for (int q = 0; q < B; ++q) {
                    void* p;
                    GDB_TRY(index_column16(ctx, (y ? ps.jy : ps.jx)[members[q]], F, &p));
                    (y ? iy : ix)[q] = p;
                }
            Pool::Lease d{pool, pool.take((int64_t)B * F * F * 8, &rc)};
            if (!d.p) return dev_fail(rc, h);
            const int e = ops.hist2d_prebinned(ctx, B, ix.data(), iy.data(), F, d.p);
            mark("binning: hist2d_prebinned done", B, F);
            if (e) return dev_fail(e, ctx);
            publish_hists(F, d.keep());
        }
        bin.launching.open();
        return 0;
    }

    // -- branch A of getAutoBandwidth2D (mcsamples.py:1347-1378): min/max of the sheared coordinate and the re-binned
    //    base grid of every sheared pair, two batched launches
    int shear_histograms(void* ctx) {
        const int base_F = s.fine_bins_2D;
        shear.A.clear();
        for (int k = 0; k < P; ++k)
            if (plan.branch[k] == 0) shear.A.push_back(k);
        shear.have = true;
        const int nA = (int)shear.A.size();
        if (!nA) return 0;
        std::vector<int32_t> ci(nA), cj(nA);
        std::vector<double> r0(nA), r1(nA), mm((size_t)2 * nA);
        for (int row = 0; row < nA; ++row) {
            const int k = shear.A[row];
            ci[row] = plan.si[k], cj[row] = plan.sj[k], r0[row] = plan.r[(size_t)2 * k], r1[row] = plan.r[(size_t)2 * k + 1];
        }
        mark("shear: start", nA);
        GDB_DEV(ctx, ops.minmax_affine(ctx, nA, ci.data(), cj.data(), r0.data(), r1.data(), mm.data()));
        mark("shear: minmax done");
        std::vector<double> xmin(nA), dx(nA), ymin(nA), dy(nA);
        shear.r1s.resize(nA), shear.r2s.resize(nA);
        for (int row = 0; row < nA; ++row) {
            const int k = shear.A[row];
            // kde.bin_samples(p1, nbins, range_min=imin, range_max=imax) (kde_bandwidth.py:76-87)
            const double mn = par[plan.si[k]].param_min, mx = par[plan.si[k]].param_max;
            const double delta = mx - mn;
            const double rmin = plan.has_imin[k] ? plan.imin[k] : mn - delta * 0.1;
            const double rmax = plan.has_imax[k] ? plan.imax[k] : mx + delta * 0.1;
            const double R1 = rmax - rmin;
            const double mn2 = mm[(size_t)2 * row], mx2 = mm[(size_t)2 * row + 1];
            const double delta2 = mx2 - mn2;
            const double rmin2 = mn2 - delta2 * 0.1;
            const double R2 = (mx2 + delta2 * 0.1) - rmin2;
            xmin[row] = rmin, dx[row] = R1 / (base_F - 1), ymin[row] = rmin2, dy[row] = R2 / (base_F - 1);
            shear.r1s[row] = R1, shear.r2s[row] = R2;
        }
        int rc = 0;
        shear.d_rot = pool.take((int64_t)nA * base_F * base_F * 8, &rc);
        if (!shear.d_rot) return dev_fail(rc, h);
        GDB_DEV(ctx, ops.hist2d_sheared(ctx, nA, ci.data(), cj.data(), r0.data(), r1.data(), xmin.data(), dx.data(), ymin.data(),
                                        dy.data(), base_F, shear.d_rot));
        mark("shear: histograms done");
        return 0;
    }

    void set_scales(const std::vector<int>& ks) {
        const double a = fabs(s.smooth_scale_2D);
        for (int k : ks) {
            rx[k] = W[(size_t)3 * k] * a / fwx[k];
            ry[k] = W[(size_t)3 * k + 1] * a / fwy[k];
            cc[k] = W[(size_t)3 * k + 2];
            finish_scale(k);
        }
    }
    void finish_scale(int k) {
        smooth[k] = np_maximum(rx[k], ry[k]);
        const double w = nearbyint(2.5 * smooth[k]);  // max(1, int(round(2.5 * smooth_scale)))
        winw[k] = (isfinite(w) && w > 1) ? (int64_t)w : 1;
        if (smooth[k] < 2) ps.warn[k] |= 2;  // "fine_bins_2D not large enough for optimal density"
    }

    // -- convolution of the pairs of one grid-size class (`only`: mask over the pairs, empty = all) on `force_ctx`, or
    //    on the stream the two-stream rules pick
    struct Batch {
        std::vector<int> pos, ks;
    };
    int class_batches(int F, const std::vector<char>& only, std::vector<Batch>& batches) {
        const std::vector<int>& members = classes.at(F);
        std::vector<int> pos_all;
        for (int q = 0; q < (int)members.size(); ++q)
            if (only.empty() || only[members[q]]) pos_all.push_back(q);
        batches.clear();
        if (pos_all.empty()) return 0;
        int64_t mb = (int64_t)(s_max_batch_bytes() / ((double)F * F * 8 * 30));
        int max_batch = (int)std::max<int64_t>(1, std::min<int64_t>(mb, s_max_batch()));
        const int first_batch = s_first_batch();
        // groups in order of first appearance; within a group sub-batches of equal frame size S >= F + 2 winw, ascending
        std::vector<int> gorder;
        for (int q : pos_all) {
            const int g = group[members[q]];
            if (std::find(gorder.begin(), gorder.end(), g) == gorder.end()) gorder.push_back(g);
        }
        for (int g : gorder) {
            std::map<int, std::vector<int>> byS;
            for (int q : pos_all) {
                const int k = members[q];
                if (group[k] != g) continue;
                const int64_t w = winw[k];
                if (w < 1 || w > 2 * (int64_t)F) return fail(GD_ERR_BADARG, "bad window half-width");
                byS[frame_size(F + 2 * (int)w)].push_back(q);
            }
            for (auto& kv : byS) {
                const std::vector<int>& cur = kv.second;
                size_t s0 = 0;
                if (batches.empty() && (int)cur.size() > first_batch) {
                    Batch b;
                    b.pos.assign(cur.begin(), cur.begin() + first_batch);
                    batches.push_back(b);
                    s0 = first_batch;
                }
                for (size_t s1 = s0; s1 < cur.size(); s1 += max_batch) {
                    Batch b;
                    b.pos.assign(cur.begin() + s1, cur.begin() + std::min(cur.size(), s1 + (size_t)max_batch));
                    batches.push_back(b);
                }
            }
        }
        for (auto& b : batches)
            for (int q : b.pos) b.ks.push_back(members[q]);
        return 0;
    }
    int s_first_batch() const { return s.first_batch > 0 ? s.first_batch : kFirstBatch; }
    int s_max_batch() const { return s.max_batch > 0 ? s.max_batch : kMaxBatch; }
    double s_max_batch_bytes() const { return s.max_batch_bytes > 0 ? s.max_batch_bytes : 24e9; }
    int s_two_min() const { return s.two_streams_min > 0 ? s.two_streams_min : 64; }
    int s_two_split() const { return s.two_streams_split > 0 ? s.two_streams_split : 400; }
    int s_kopt_split_min() const { return s.kopt_split_min > 0 ? s.kopt_split_min : 256; }

    bool is_side(int F) const { return std::find(conv.side_classes.begin(), conv.side_classes.end(), F) != conv.side_classes.end(); }

    // (the up-scaled classes' buffers arrive with the deferred chain: null until then)
    void* class_buffer(int F) {
        std::lock_guard<std::mutex> g(enq_mu);
        auto it = hists.find(F);
        return it == hists.end() ? nullptr : it->second;
    }

    int enqueue_batch(int F, const Batch& b, void* force_ctx) {
        const std::vector<int>& members = classes.at(F);
        void* bctx;
        if (force_ctx)
            bctx = force_ctx;
        else if (!conv.side_classes.empty() || P > s_two_split())
            bctx = conv.ctxs[is_side(F) && conv.ctxs.size() > 1 ? 1 : 0];
        else
            bctx = conv.ctxs[conv.batch_no % conv.ctxs.size()];
        ++conv.batch_no;
        const int B = (int)b.pos.size();
        const int64_t item = (int64_t)F * F * 8;
        void* d_hist = class_buffer(F);  // (under enq_mu: the deferred shear chain may be adding the up-scaled classes' buffers)
        if (!d_hist) return fail(GD_ERR_BADARG, "a grid-size class has no histograms");
        int rc = 0;
        bool whole = B == (int)members.size();
        for (int q = 0; q < B && whole; ++q) whole = b.pos[q] == q;
        // (a batch that is not the whole class convolves its histograms where they lie: the kernels take an index list)
        std::vector<int32_t> hidx(b.pos.begin(), b.pos.end());
        std::vector<double> rxb(B), ryb(B), ccb(B);
        std::vector<int32_t> wb(B), fb(B);
        for (int q = 0; q < B; ++q) {
            const int k = b.ks[q];
            rxb[q] = rx[k], ryb[q] = ry[k], ccb[q] = cc[k], wb[q] = (int32_t)winw[k], fb[q] = flags[k];
        }
        void* d_P = pool.take((int64_t)B * item, &rc);
        if (!d_P) return dev_fail(rc, h);
        conv.call_blocks.push_back(d_P);
        int32_t* status = status_pinned + conv.status_at;
        for (int q = 0; q < B; ++q) status[q] = kStatusPending;  // (overwritten by the batch's last launch: see Conv::first_run_word)
        if (conv.grid_off + (int64_t)B * F * F > grids_doubles) return fail(GD_ERR_BADARG, "grids_pinned is too small");
        mark(bctx == h ? "conv: enqueue on main" : "conv: enqueue on twin", B, F);
        GDB_DEV(bctx, ops.density2d_enqueue(bctx, B, F, d_hist, whole ? nullptr : hidx.data(), rxb.data(), ryb.data(), ccb.data(),
                                            wb.data(), fb.data(), s.boundary_correction_order, s.mult_bias_correction_order, d_P,
                                            status));
        mark("conv: enqueued");
        if (s.want_levels && levels) {
            std::vector<double> lv((size_t)B * s.ncontours);
            std::vector<int32_t> ls(B);
            GDB_DEV(bctx, ops.contour_levels(bctx, B, F, d_P, s.contours, s.ncontours, lv.data(), ls.data()));
            for (int q = 0; q < B; ++q) {
                memcpy(levels + (size_t)b.ks[q] * s.ncontours, &lv[(size_t)q * s.ncontours], sizeof(double) * s.ncontours);
                level_status[b.ks[q]] = ls[q];
            }
        }
        GDB_DEV(bctx, ops.d2h_async(bctx, grids + conv.grid_off, d_P, (int64_t)B * item));
        for (int q = 0; q < B; ++q) {
            double* m = M(b.ks[q]);
            m[1] = (double)(conv.grid_off + (int64_t)q * F * F);
            m[29] = bctx == twin ? 1.0 : 0.0;
            m[30] = (double)(conv.status_at + q);
        }
        conv.grid_off += (int64_t)B * F * F;
        conv.status_at += B;
        return 0;
    }

    int run_class(int F, const std::vector<char>& only, void* force_ctx) {
        std::vector<Batch> batches;
        GDB_TRY(class_batches(F, only, batches));
        for (const Batch& b : batches) GDB_TRY(enqueue_batch(F, b, force_ctx));
        return 0;
    }

    // every class, all pairs: classes that go to the second stream are queued there right after the main class's first batch
    int enqueue_all() {
        std::vector<int> main_, side;
        for (int F : conv.order) (is_side(F) ? side : main_).push_back(F);
        const std::vector<char> all;
        std::vector<Batch> first;
        size_t first_done = 0;
        if (!side.empty() && !main_.empty()) {
            GDB_TRY(class_batches(main_[0], all, first));
            if (!first.empty()) {
                GDB_TRY(enqueue_batch(main_[0], first[0], nullptr));
                first_done = 1;
            }
        }
        for (int F : side) GDB_TRY(run_class(F, all, nullptr));
        for (size_t q = 0; q < main_.size(); ++q) {
            if (q == 0 && !side.empty()) {
                for (size_t b = first_done; b < first.size(); ++b) GDB_TRY(enqueue_batch(main_[0], first[b], nullptr));
                continue;
            }
            GDB_TRY(run_class(main_[q], all, nullptr));
        }
        return 0;
    }

    // -- getAutoBandwidth2D for the batch (mcsamples.py:1325-1419): the optimiser's launches (plan_launches), unit
    //    conversions, de-rotation of the sheared kernels, fallbacks, widening; on_chunk(ks, index of the launch, number of
    //    launches) after every launch.
    //    Sequential: every launch is one blocking gd_kopt2d call on the main context.
    //    Staged (large calls with a second and a third stream): the base grid's pairs are cut into parts; the calling thread
    //    enqueues stage A of every part (DCT, fixed point, functionals) back to back on the main stream, a second thread runs
    //    stage B (get_h: the serial TNC minimisations) of part k on the third stream -- beside stage A of part k + 1 -- and a
    //    third hands the part's final bandwidths to on_chunk, which enqueues its convolution.
    typedef std::function<int(const std::vector<int>&, int, int)> ChunkFn;
    typedef std::function<int(std::vector<int>, int)> ReportFn;

    // a launch that holds sheared rows, or belongs to a class the deferred chain bins, waits for that chain here
    int ready_for(Launch& L) {
        if (L.na > 0 && L.d_hist && shear.running) {
            // the sheared rows are all this launch is waiting for (its own class has its buffer)
            const bool opened = shear.hists.wait(20, 0);
            mark("shear: histograms awaited");
            if (!opened || shear.hists.code()) {
                const int e = join_shear();
                return e ? e : GD_ERR_HIP;
            }
        } else if (L.na > 0 || !L.d_hist) {
            GDB_TRY(join_shear());
            if (!L.d_hist) L.d_hist = class_buffer(L.F);
            if (!L.d_hist) return fail(GD_ERR_BADARG, "a grid-size class has no histograms");
        }
        return 0;
    }
    // a launch of the base class whose rows the FIRST binning launch has filled may go ahead of the second
    bool rows_binned_first(const Launch& L) const {
        if (bin.first_rows <= 0 || L.F != s.fine_bins_2D || L.na > 0 || !L.d_hist) return false;
        for (int q : L.pos)
            if (q >= bin.first_rows) return false;
        return true;
    }
    int whole_binning_for(Launch& L) {
        GDB_TRY(join_binning());
        if (L.F == s.fine_bins_2D && !L.pos.empty())  // (a class buffer whose second launch failed has been replaced)
            if (void* p = class_buffer(L.F)) L.d_hist = p;
        return 0;
    }

    int build_batch(Launch& L) {  // the launch's histograms as one device block (a gather unless the class buffer serves)
        const int B = (int)L.ks.size(), F = L.F;
        const int64_t item = (int64_t)F * F * 8;
        L.d_batch = L.d_hist, L.own = false;
        if (!L.whole) {
            int rc = 0;
            L.d_batch = pool.take((int64_t)B * item, &rc);
            if (!L.d_batch) return dev_fail(rc, h);
            L.own = true;
            if (L.na) {
                std::vector<int32_t> idx(L.na);
                for (int a = 0; a < L.na; ++a) idx[a] = a;
                GDB_DEV(h, ops.gather_items(h, L.d_batch, 0, shear.d_rot, idx.data(), L.na, item));
            }
            if (!L.pos.empty()) {
                std::vector<int32_t> idx(L.pos.begin(), L.pos.end());
                GDB_DEV(h, ops.gather_items(h, L.d_batch, L.na, L.d_hist, idx.data(), (int)idx.size(), item));
            }
        }
        L.ne.resize(B), L.fb.resize(B), L.ci.resize(B), L.dc.resize(B);
        for (int row = 0; row < B; ++row) {
            const int k = L.ks[row];
            const bool rowA = row < L.na;
            L.ne[row] = plan.neff[k], L.dc[row] = plan.has_limits[k] ? 0 : 1;
            L.fb[row] = rowA ? -1.0 : plan.fallback_t[k];
            L.ci[row] = rowA ? 0.0 : ps.actual[k];
        }
        return 0;
    }

    // the optimiser's rows of one launch -> bandwidths in parameter units (W), records, fallbacks
    int absorb_rows(const Launch& L, const std::vector<double>& out) {
        const int B = (int)L.ks.size();
        for (int row = 0; row < B; ++row) {
            const double* o = &out[(size_t)row * 12];
            if (o[7] == 0 && o[11] != 0) return fail(GD_ERR_BADARG, "bias not positive definite");  // kde_bandwidth.py:229-230, out of get_h
        }
        for (int row = 0; row < B; ++row) {
            const int k = L.ks[row];
            const double* o = &out[(size_t)row * 12];
            memcpy(M(k) + 6, o, 12 * sizeof(double));
            double hx, hy, c;
            if (row < L.na) {
                // de-rotate the sheared kernel (mcsamples.py:1379-1390): kernelC = S K S^T for the 2 x 2 case
                const double hxa = o[8] * shear.r1s[row], hya = o[9] * shear.r2s[row], ca = o[10];
                const double* S = &plan.S[(size_t)4 * k];
                const double k00 = hxa * hxa, k01 = hxa * hya * ca, k11 = hya * hya;
                const double t00 = S[0] * k00 + S[1] * k01, t01 = S[0] * k01 + S[1] * k11;
                const double t10 = S[2] * k00 + S[3] * k01, t11 = S[2] * k01 + S[3] * k11;
                const double c00 = t00 * S[0] + t01 * S[1], c01 = t00 * S[2] + t01 * S[3], c11 = t10 * S[2] + t11 * S[3];
                const double sx = sqrt(c00), sy = sqrt(c11);
                hx = plan.swap[k] ? sy : sx, hy = plan.swap[k] ? sx : sy, c = c01 / sqrt(c00 * c11);
            } else {
                hx = o[8] * plan.rangex[k], hy = o[9] * plan.rangey[k], c = o[10];
            }
            if (o[7] != 0) {  // "2D fixed point: no root in [0, 0.1]": the fallback widths (mcsamples.py:1402-1409)
                if (s.raise_on_bandwidth_errors) {
                    char buf[200];
                    snprintf(buf, sizeof buf, "2D kernel density bandwidth optimizer failed for pair %d (columns %d, %d). "
                             "Using fallback width: 2D fixed point: no root in [0, 0.1]", k, (int)ps.jx[k], (int)ps.jy[k]);
                    return fail(GD_ERR_SOLVER, buf);
                }
                ps.warn[k] |= 4;
                const double d = py_pow(plan.neff[k], 1.0 / 6);
                hx = par[ps.jx[k]].sigma_range / d, hy = par[ps.jy[k]].sigma_range / d;
                c = std::max(std::min(ps.actual[k], s.max_corr_2D), -s.max_corr_2D);
            }
            W[(size_t)3 * k] = hx, W[(size_t)3 * k + 1] = hy, W[(size_t)3 * k + 2] = c;
        }
        return 0;
    }

    // which parts' convolutions go to the main stream (behind the optimiser's stage A there): the last two fifths
    static bool part_on_main(int index, int nparts) { return nparts > 1 && index >= nparts - std::max(1, 2 * nparts / 5); }

    int run_sequential(std::vector<Launch>& launches, const ReportFn& report) {
        const int nl = (int)launches.size();
        int rc = join_binning();
        for (int q = 0; q < nl && !rc; ++q) {
            Launch& L = launches[q];
            const int B = (int)L.ks.size();
            std::vector<double> out((size_t)B * 12);
            rc = guarded([&]() -> int {
                GDB_TRY(whole_binning_for(L));
                GDB_TRY(ready_for(L));
                GDB_TRY(build_batch(L));
                mark("kopt: launch", B, L.F);
                const int e = ops.kopt2d(h, B, L.F, L.d_batch, L.ne.data(), L.dc.data(), L.fb.data(), L.ci.data(), out.data());
                mark("kopt: done");
                return e ? dev_fail(e, h) : 0;
            });
            if (L.own) pool.give(L.d_batch);  // (the entry point has waited for its kernels)
            if (!rc) rc = absorb_rows(L, out);
            if (!rc) rc = report(L.ks, q);
        }
        if (!rc && nl == 0) rc = report({}, 0);
        return rc;
    }

    // stage A of every launch from this thread, stage B from a second one, the convolutions from a third
    int run_staged(std::vector<Launch>& launches, const ReportFn& report) {
        const int nl = (int)launches.size();
        std::mutex mu;
        std::condition_variable cv;
        int n_staged = 0;
        bool abort_ = false;
        // Hand-over of finished parts: the finisher only runs stage B; a third thread enqueues a part's convolution.  When
        // the finisher did both, the get_h launch of part k + 1 waited for the ~2 ms of host work that enqueueing part k's
        // ~120 convolution launches takes (trace: stage A of part 2 done at 18.9 ms, its get_h started at 22.9), and the
        // convolutions of the later parts were launch-bound behind it.
        std::deque<int> handed;  // parts whose bandwidths are final, in order; -1: no more
        auto hand = [&](int q) {
            std::lock_guard<std::mutex> g(mu);
            handed.push_back(q);
            cv.notify_all();
        };
        Worker enqueuer, finisher;
        enqueuer.result = start(h, [&]() -> int {
            int e = 0;
            for (;;) {
                int q;
                {
                    std::unique_lock<std::mutex> g(mu);
                    cv.wait(g, [&] { return !handed.empty(); });
                    q = handed.front();
                    handed.pop_front();
                }
                if (q < 0) return e;
                if (e) continue;
                if (part_on_main(q, nl) || !shear.deferred) {
                    // this part's convolution uses the main context: the staging thread must be done with it.  (The
                    // earlier parts go to the second context only -- with the deferred shear chain the staging thread
                    // may still be waiting for that chain when the first part's bandwidths are final, and the first
                    // part's grids are what the result copies start with.)
                    std::unique_lock<std::mutex> g(mu);
                    cv.wait(g, [&] { return n_staged >= nl || abort_; });
                    if (n_staged < nl) {
                        e = GD_ERR_HIP;  // (the staging thread gave up: its error is the call's)
                        continue;
                    }
                }
                e = join_binning();  // (long done by now: a report may convolve any row of the class)
                if (!e) e = report(launches[q].ks, q);
                if (conv.reports_enqueued++ == 0 && conv.status_at > 0 && !s.results_in_flight)
                    conv.first_run_word.store(status_pinned + conv.status_at - 1);  // the last word of the first report's last batch
                conv.first_enqueued.open();
            }
        });
        finisher.result = start(aux, [&]() -> int {
            // (whatever ends this thread: the chain is released and the enqueuer learns that no more parts come)
            const AtExit last{[&] {
                conv.first_enqueued.open();
                hand(-1);
            }};
            int e = 0;
            for (int q = 0; q < nl; ++q) {
                {
                    std::unique_lock<std::mutex> g(mu);
                    cv.wait(g, [&] { return n_staged > q || abort_; });
                    if (n_staged <= q) break;  // (the staging thread gave up)
                }
                Launch& L = launches[q];
                const int B = (int)L.ks.size();
                std::vector<double> out((size_t)B * 12);
                if (!e) {
                    e = guarded([&] { return ops.kopt2d_finish(aux, h, L.ticket, B, L.d_rows, out.data()); });
                    mark("kopt: part finished", q, B);
                    if (e) dev_fail(e, aux);
                } else {
                    ops.copy_sync(h);  // (never reached in a healthy run: blocks are not freed under running kernels)
                }
                // stage B has waited for stage A: the part's input blocks are free
                if (L.own) pool.give(L.d_batch);
                pool.give(L.d_rows);
                if (!e) e = absorb_rows(L, out);
                if (e) conv.first_enqueued.open();
                if (!e) hand(q);
            }
            return e;
        });
        int rc = 0;
        {
            // (whatever ends the staging: parts that were never staged are not waited for)
            const AtExit give_up{[&] {
                std::lock_guard<std::mutex> g(mu);
                if (n_staged < nl) abort_ = true;
                cv.notify_all();
            }};
            for (int q = 0; q < nl && !rc; ++q) {
                Launch& L = launches[q];
                const int B = (int)L.ks.size();
                rc = guarded([&]() -> int {
                    if (!(q == 0 && rows_binned_first(L))) GDB_TRY(whole_binning_for(L));
                    GDB_TRY(ready_for(L));
                    GDB_TRY(build_batch(L));
                    int e = 0;
                    L.d_rows = pool.take((int64_t)B * GD_KOPT_BLOCK_DOUBLES * 8, &e);
                    if (!L.d_rows) return dev_fail(e, h);
                    mark("kopt: stage A enqueue", q, B);
                    e = ops.kopt2d_enqueue(h, B, L.F, L.d_batch, L.ne.data(), L.dc.data(), L.fb.data(), L.ci.data(), L.d_rows, &L.ticket);
                    return e ? dev_fail(e, h) : 0;
                });
                std::lock_guard<std::mutex> g(mu);
                if (rc) {
                    if (L.own && L.d_batch) ops.copy_sync(h), pool.give(L.d_batch);
                    if (L.d_rows) pool.give(L.d_rows);
                } else {
                    ++n_staged;
                }
                cv.notify_all();
            }
        }
        mark("kopt: every stage A enqueued");
        const int e = finisher.join();
        const int e2 = enqueuer.join();
        if (!rc) rc = e;
        if (!rc) rc = e2;
        return rc;
    }

    int bandwidth_2d(bool staged, const ChunkFn& on_chunk) {
        const int base_F = s.fine_bins_2D;
        const int m = s.mult_bias_correction_order;
        std::vector<double> widen;
        if (m) {
            widen.resize(P);
            const double e = 1.0 / 6 - 1.0 / (2 + 4 * (1 + m));
            for (int k = 0; k < P; ++k) widen[k] = 1.1 * py_pow(plan.neff[k], e);
        }
        if (!shear.deferred && !shear.have) GDB_TRY(shear_histograms(h));  // (a deferred chain is still writing `have`)
        std::vector<int> waiting;
        for (int k = 0; k < P; ++k)
            if (plan.branch[k] == 1) {  // rule of thumb (mcsamples.py:1391-1395)
                const double c = std::max(std::min(ps.actual[k], s.max_corr_2D), -s.max_corr_2D);
                const double d = py_pow(plan.neff[k], 1.0 / 6);
                W[(size_t)3 * k] = par[ps.jx[k]].sigma_range / d, W[(size_t)3 * k + 1] = par[ps.jy[k]].sigma_range / d, W[(size_t)3 * k + 2] = c;
                waiting.push_back(k);
            }
        std::vector<Launch> launches = plan_launches(plan.branch, F_list, classes, base_F, staged, shear.deferred, s_kopt_split_min());
        const int nl = (int)launches.size();
        for (Launch& L : launches) {
            if (L.pos.empty()) {  // the sheared pairs alone: their histograms are the buffer
                GDB_TRY(join_shear(true));
                L.d_hist = shear.d_rot;
            } else {
                L.d_hist = class_buffer(L.F);
            }
        }
        // (the deferred shear chain waits for the first part's convolution -- unless that part itself waits for the chain)
        if (!staged || nl == 0 || launches[0].na > 0 || !launches[0].d_hist) conv.first_enqueued.open();
        ReportFn report = [&](std::vector<int> ks, int index) -> int {
            if (!waiting.empty()) {
                // the rule-of-thumb pairs ride with the first report -- except, with the deferred shear chain, those of a
                // class that chain bins (an up-scaled grid): they wait for the last report, when the chain has been joined
                std::vector<int> all, later;
                for (int k : waiting) ((shear.deferred && ps.F[k] != base_F && index + 1 < nl) ? later : all).push_back(k);
                all.insert(all.end(), ks.begin(), ks.end());
                ks.swap(all);
                waiting.swap(later);
            }
            if (m)
                for (int k : ks) W[(size_t)3 * k] *= widen[k], W[(size_t)3 * k + 1] *= widen[k];
            // the last report convolves the rule-of-thumb pairs of the classes the chain bins: the WHOLE chain, not only
            // its sheared histograms (ready_for), has to be through
            if (shear.deferred && index + 1 >= nl) GDB_TRY(join_shear());
            if (!ks.empty() || index + 1 >= nl) return on_chunk(ks, index, nl);
            return 0;
        };
        int rc = (!staged || nl == 0) ? run_sequential(launches, report) : run_staged(launches, report);
        {
            const int e0 = join_binning();
            const int e = join_shear(true);  // (an error path may get here before any launch asked for it)
            if (!rc) rc = e0;
            if (!rc) rc = e;
        }
        if (shear.d_rot) pool.give(shear.d_rot), shear.d_rot = nullptr;
        return rc;
    }

    // -- the O(N) phase of a large call.  Three streams are busy from the start: the N_eff kernels (fp64 exp-bound) on the
    //    main context, the byte-index binning (LDS atomics) on the second, the sheared min/max + re-binning (HBM-bound) on
    //    a third the library creates for itself; the per-pair scalars and the branch plan are worked out meanwhile.
    void start_neff_thread() {
        bin.hold_neff = unit_weights;
        neff.result = start(h, [this] { return neff_batch(used, true); });
    }
    // the deferred chain (see Shear): large unit-weight calls; it needs the fourth context
    void choose_shear_mode() {
        shear.deferred = env.shear_deferred && unit_weights && P >= env.shear_deferred_min;
        // (measured: the chain's stream at the LOWEST priority, so that the optimiser's blocks would be dispatched ahead of it
        // -- 30.0-30.4 ms per delivered triangle against 29.5-29.7 with the high priority create_aux gives it, 30.6-30.8 with
        // the chain joined in front of the optimiser: its 1024-thread blocks hold their CUs either way, and a low priority
        // only delays the chain's end)
        if (shear.deferred && !st.aux2 && ops.create_aux(h, &st.aux2)) {
            if (st.aux2) ops.destroy_aux(st.aux2), st.aux2 = nullptr;
            shear.deferred = false, (void)ops.last_error(h);
        }
    }
    // the rows of the main class that the first binning launch fills: the first optimiser part's (see Binning)
    void plan_first_binning_rows() {
        const bool will_stage = aux != nullptr && !s.want_levels && P >= s_two_min() && P > s_two_split() && !s.bandwidths_only;
        if (!(shear.deferred && will_stage && s.fine_bins_2D == 256 && main_class() == 256 && !env.one_binning)) return;
        std::vector<int>& mem = classes[256];
        std::stable_partition(mem.begin(), mem.end(), [&](int k) { return plan.branch[k] == 2; });
        size_t nC = 0, nA = 0;
        for (int k : mem) nC += plan.branch[k] == 2;
        for (int k = 0; k < P; ++k) nA += plan.branch[k] == 0;
        if ((int)nC < s_kopt_split_min()) return;
        // (measured: a first part of 256 pairs, the others unchanged -- delivered 27.2-27.6 against 27.3-27.7 ms, the stream of
        // triangles 21.0-21.2 against 20.6-20.7: the result copies saturate PCIe from the first batch on and the copy engine
        // then waits for the second part.  So the first part is a part like the others.)
        const size_t part = base_part_size(nC + nA, 256, s_kopt_split_min()), first = std::min(nC, part);
        if (nC + nA > part && first < mem.size()) bin.first_rows = (int)first;
    }
    void start_binning_thread(bool split_classes) {
        bin.thread.result = start(twin, [this, split_classes] { return binning(twin, split_classes ? 1 : 0); }, &bin.first_run, &bin.done);
    }
    // What the deferred chain holds for before it takes the machine: the whole main binning has run, the first optimiser
    // part's convolution is enqueued and -- where that is the signal (Conv::first_run_word) -- has run.  Every wait is bounded.
    void hold_chain_start() {
        bin.done.wait(50, 50000);
        conv.first_enqueued.wait(50, 20000);
        if (const volatile int32_t* word = conv.first_run_word.load())
            poll_until([word] { return *word != kStatusPending; }, 20, 20000);
        mark("shear: main binning has run, first part's bandwidths final");
    }
    void start_shear_chain(bool split_classes) {
        void* sctx = shear.deferred ? st.aux2 : aux;
        shear.thread.result = start(sctx, [this, sctx, split_classes] {
            if (shear.deferred) hold_chain_start();
            const int e = shear_histograms(sctx);
            shear.hists.open(e);
            if (env.side_binning_delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(env.side_binning_delay_ms));
            const int e2 = split_classes ? binning(sctx, 2) : 0;  // the up-scaled classes, behind the shear chain
            return e ? e : e2;
        }, &shear.hists);
    }
    // N_eff, the plan's second half, the chain (unless deferred) and the binning -- of the first optimiser part's rows only
    // where the main class is binned in two launches: whoever needs more joins the binning (bandwidth_2d)
    int join_linear_phase(int rc, bool* exchanged) {
        int e = neff.join();
        if (!rc) rc = e;
        if (!rc) rc = neff_complete(exchanged);  // (multi-rank: the other ranks' values, from this thread)
        if (!rc) fill_plan(par, ps, plan, s.pair_neff);
        if (shear.deferred) {
            shear.running = shear.thread.result.valid();  // joined by the first launch that needs it
        } else {
            e = join_shear();
            if (!rc) rc = e;
        }
        if (bin.first_rows > 0 && !rc && bin.first_run.wait(20, 0) && bin.first_run.code() == 0) {
            mark("binning: first part's rows done", bin.first_rows);
        } else {
            e = join_binning();
            if (!rc) rc = e;
        }
        if (rc) (void)join_shear(true);
        return rc;
    }

    int run(int32_t* tokens_out2) {
        const int rc = guarded([&] { return run_steps(tokens_out2); });
        return rc ? cleanup(rc) : 0;
    }
    int run_steps(int32_t* tokens_out2) {
        tokens_out2[0] = tokens_out2[1] = -1;
        const int base_F = s.fine_bins_2D, bco = s.boundary_correction_order;
        const double ss = s.smooth_scale_2D;
        if (fabs(s.max_corr_2D) > 1) return fail(GD_ERR_BADARG, "max_corr_2D cannot be >=1");
        if (bco > 1) return fail(GD_ERR_BADARG, "unknown boundary_correction_order (expected 0 or 1)");
        if (base_F < 8 || base_F > 4096) return fail(GD_ERR_BADARG, "fine_bins_2D out of range");
        bool exchanged = false;
        if (P == 0) {  // (a rank without pairs still takes part in the exchange)
            GDB_TRY(neff_exchange(&exchanged));
            return 0;
        }
        mark("call: start", P);
        int64_t ncols = 0;
        GDB_DEV(h, ops.num_rows(h, &N, &ncols));
        if (ncols < n) return fail(GD_ERR_BADARG, "more parameters than resident columns");
        int32_t hw = 0;
        GDB_DEV(h, ops.weights_kind(h, &hw));
        unit_weights = hw == 0;
        byte_index_weights = hw == 2 && !env.no_wsort;
        for (int k = 0; k < P; ++k)
            if (pairs[2 * k] < 0 || pairs[2 * k] >= n || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= n)
                return fail(GD_ERR_BADARG, "pair index out of range");
        {  // columns in order of first appearance
            std::vector<char> seen(n, 0);
            for (int k = 0; k < 2 * P; ++k)
                if (!seen[pairs[k]]) seen[pairs[k]] = 1, used.push_back(pairs[k]);
        }
        // settings->bandwidths: the caller's (hx, hy, corr) per pair instead of getAutoBandwidth2D (tests inject the
        // oracle's triples); settings->pair_neff: the caller's effective sample number per pair (use_effective_samples_2D)
        const bool injected = ss < 0 && s.bandwidths != nullptr;
        const bool auto_bw = ss < 0 && !injected;
        bool need_neff = false;
        if (auto_bw && !s.pair_neff)
            for (int j : used) need_neff = need_neff || isnan(par[j].neff);
        const bool overlap = auto_bw && P >= 64 && twin != nullptr;  // a large call: see start_neff_thread
        if (overlap) {
            if (!st.aux) GDB_DEV(h, ops.create_aux(h, &st.aux));
            aux = st.aux;
            if (need_neff) start_neff_thread();
        }
        bmin.assign(n, NAN), bmax.assign(n, NAN);
        for (int j : used) bin_edges(par[j], &bmin[j], &bmax[j]);
        pair_scalars(s, n, corrmat, pairs, P, ps);
        fwx.resize(P), fwy.resize(P);
        for (int k = 0; k < P; ++k) {
            const int F = ps.F[k];
            if (!classes.count(F)) F_list.push_back(F);
            classes[F].push_back(k);
            fwx[k] = (bmax[ps.jx[k]] - bmin[ps.jx[k]]) / (F - 1);
            fwy[k] = (bmax[ps.jy[k]] - bmin[ps.jy[k]]) / (F - 1);
            double* m = M(k);
            for (int q = 0; q < GD_BATCH2D_META; ++q) m[q] = NAN;
            m[0] = F, m[5] = -1, m[23] = bmin[ps.jx[k]], m[24] = bmax[ps.jx[k]], m[25] = bmin[ps.jy[k]], m[26] = bmax[ps.jy[k]];
            m[27] = ps.corr[k], m[28] = (double)ps.nbin2D[k];
        }
        int64_t need = 0;
        for (int k = 0; k < P; ++k) need += (int64_t)ps.F[k] * ps.F[k];
        if (need > grids_doubles && !s.bandwidths_only) {
            (void)neff.join();
            return fail(GD_ERR_BADARG, "grids_pinned is too small");
        }
        std::vector<double> rngx(P), rngy(P);
        for (int k = 0; k < P; ++k) rngx[k] = bmax[ps.jx[k]] - bmin[ps.jx[k]], rngy[k] = bmax[ps.jy[k]] - bmin[ps.jy[k]];
        int rc = 0;
        if (auto_bw && overlap) {
            const bool split_classes = F_list.size() > 1;
            choose_shear_mode();
            rc = make_plan(s, par, n, cov, ps, rngx, rngy, 0.2, plan, err);  // (needs the limits and the covariance only)
            if (!rc) plan_first_binning_rows();
            start_binning_thread(split_classes);
            if (!rc) start_shear_chain(split_classes);  // (no plan: the call fails; the side classes are not needed)
            rc = join_linear_phase(rc, &exchanged);
        } else if (auto_bw) {
            rc = s.pair_neff ? 0 : neff_batch(used, true);
            if (!rc) rc = neff_complete(&exchanged);
            if (!rc) rc = binning(h);
            if (!rc) rc = make_plan(s, par, n, cov, ps, rngx, rngy, 0.2, plan, err);
            if (!rc) fill_plan(par, ps, plan, s.pair_neff);
        } else {
            rc = neff_exchange(&exchanged);  // the collective is unconditional: once per call on every rank
            if (!rc && !s.bandwidths_only) rc = binning(h);
        }
        mark("binning / N_eff / plan joined");
        if (rc) return rc;
        // ---- convolution set-up: flag bits (mcsamples.py:1688-1703, 1794): bits 0/1 = x bot/top, 2/3 = y bot/top,
        //      4/5 = x/y periodic, 6 = has_prior
        flags.resize(P), group.resize(P);
        for (int k = 0; k < P; ++k) {
            const gd_param2d &px = par[ps.jx[k]], &py = par[ps.jy[k]];
            const int lbx = px.periodic ? 0 : (px.has_limits_bot ? 1 : 0) | (px.has_limits_top ? 2 : 0);
            const int lby = py.periodic ? 0 : (py.has_limits_bot ? 1 : 0) | (py.has_limits_top ? 2 : 0);
            const int has_prior = has_limits(px) || has_limits(py);
            flags[k] = lbx | ((px.periodic ? 1 : 0) << 4) | (lby << 2) | ((py.periodic ? 1 : 0) << 5) | (has_prior << 6);
            group[k] = (flags[k] & 48) * 2 + ((has_prior && bco >= 0) ? 1 : 0);
        }
        rx.assign(P, NAN), ry.assign(P, NAN), cc.assign(P, NAN), smooth.assign(P, NAN), winw.assign(P, 0), W.assign((size_t)3 * P, NAN);
        const bool lazy = !s.want_levels;
        conv.ctxs = {h};
        if (lazy && twin && P >= s_two_min()) {
            if (P > s_two_split()) {
                for (int F : F_list)
                    if ((int)classes.at(F).size() < 64) conv.side_classes.push_back(F);
                if (conv.side_classes.size() == F_list.size()) conv.side_classes.clear();
            }
            conv.ctxs.push_back(twin);
        }
        // largest class (in bytes) first: the copy of the last, smallest one is the only exposed one
        conv.order = F_list;
        std::stable_sort(conv.order.begin(), conv.order.end(), [&](int a, int b) {
            return (int64_t)classes.at(a).size() * a * a > (int64_t)classes.at(b).size() * b * b;
        });
        std::vector<int> all_k(P);
        for (int k = 0; k < P; ++k) all_k[k] = k;
        if (auto_bw) {
            const bool staged = aux != nullptr && conv.ctxs.size() > 1 && P > s_two_split() && !s.bandwidths_only;
            if (staged) {
                // every part's convolution is enqueued (by the thread that finishes the parts) as soon as its bandwidths are
                // final: the first parts on the second stream, beside the optimiser's stage A of the later parts on the
                // main stream; the last parts behind stage A on the main stream, so that both streams end together
                ChunkFn on_chunk = [&](const std::vector<int>& ks, int index, int nparts) -> int {
                    set_scales(ks);
                    std::vector<char> only(P, 0);
                    for (int k : ks) only[k] = 1;
                    const bool to_main = part_on_main(index, nparts);
                    // (measured alternatives, C3 step: every part on the second stream 31.4 ms, the last parts on the third
                    // -- high-priority -- stream 36.3 ms, against 30.4 ms as below)
                    for (int F : conv.order) {
                        void* target = (is_side(F) || !to_main) ? conv.ctxs[1] : conv.ctxs[0];
                        GDB_TRY(run_class(F, only, target));
                    }
                    return 0;
                };
                rc = bandwidth_2d(true, on_chunk);
            } else {
                ChunkFn on_chunk = [&](const std::vector<int>&, int, int) -> int { return 0; };
                rc = bandwidth_2d(false, on_chunk);
                if (!rc) {
                    set_scales(all_k);
                    if (!s.bandwidths_only) rc = enqueue_all();
                }
            }
            for (int k = 0; k < P && !rc; ++k) {
                double* m = M(k);
                m[2] = W[(size_t)3 * k], m[3] = W[(size_t)3 * k + 1], m[4] = W[(size_t)3 * k + 2];
                m[5] = plan.branch[k], m[31] = plan.neff[k];
            }
        } else if (injected) {
            for (int k = 0; k < P; ++k) {
                for (int q = 0; q < 3; ++q) W[(size_t)3 * k + q] = s.bandwidths[(size_t)3 * k + q];
                double* m = M(k);
                m[2] = W[(size_t)3 * k], m[3] = W[(size_t)3 * k + 1], m[4] = W[(size_t)3 * k + 2];
            }
            set_scales(all_k);
            if (!s.bandwidths_only) rc = enqueue_all();
        } else {
            for (int k = 0; k < P; ++k) {
                if (ss < 1.0) {
                    rx[k] = ss * par[ps.jx[k]].err / fwx[k];
                    ry[k] = ss * par[ps.jy[k]].err / fwy[k];
                } else {
                    rx[k] = ry[k] = ss * ps.F[k] / (double)ps.nbin2D[k];
                }
                cc[k] = ps.corr[k];
                finish_scale(k);
            }
            if (!s.bandwidths_only) rc = enqueue_all();
        }
        if (rc) return rc;
        for (int k = 0; k < P; ++k) {
            double* m = M(k);
            m[18] = rx[k], m[19] = ry[k], m[20] = cc[k], m[21] = (double)winw[k], m[22] = ps.warn[k];
        }
        mark("all batches enqueued");
        class_buffers_to_call_blocks();
        GDB_DEV(h, ops.copy_mark(h, &tokens_out2[0]));
        if (conv.ctxs.size() > 1) GDB_DEV(twin, ops.copy_mark(twin, &tokens_out2[1]));
        if (!lazy) {
            for (void* c : conv.ctxs) GDB_DEV(c, ops.copy_sync(c));
            for (void* p : conv.call_blocks) pool.give(p);
            conv.call_blocks.clear();
            return 0;
        }
        // This call's blocks wait for its copies.  The previous call's copies are ahead of this call's on the copy
        // streams: completing it here costs no waiting, and its device blocks return to the pool even if nobody ever
        // read its grids.
        Pending cur;
        cur.blocks.swap(conv.call_blocks);
        cur.tok_main = tokens_out2[0], cur.tok_twin = tokens_out2[1], cur.twin = conv.ctxs.size() > 1 ? twin : nullptr;
        cur.live = true;
        const int e_prev = complete_pending(st, ops, h, st.prev);
        st.prev = std::move(cur);
        mark("previous call completed; return");
        dump_timeline();
        if (e_prev) return dev_fail(e_prev, h);
        return 0;
    }

    void class_buffers_to_call_blocks() {  // (released with the call's other blocks)
        for (auto& kv : hists) conv.call_blocks.push_back(kv.second);
        hists.clear();
        conv.call_blocks.insert(conv.call_blocks.end(), bin.stale.begin(), bin.stale.end());
        bin.stale.clear();
    }
    // an error after device work was started: wait for whatever is in flight, hand every block back
    int cleanup(int rc) {
        (void)neff.join();
        (void)join_binning();
        (void)join_shear(true);  // (a deferred chain still running on its own context uses the pool and the class table)
        ops.copy_sync(h);
        if (twin) ops.copy_sync(twin);
        class_buffers_to_call_blocks();
        if (shear.d_rot) pool.give(shear.d_rot), shear.d_rot = nullptr;
        for (void* p : conv.call_blocks) pool.give(p);
        conv.call_blocks.clear();
        return rc;
    }
#undef GDB_DEV
#undef GDB_TRY
};

}  // namespace gdb

