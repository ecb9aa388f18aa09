// The launch arithmetic of stats.hip in one place (plain C++17, no HIP: compiles with g++ like binplan.hpp;
// tests/native/statsplan_check.cpp sweeps it).  Every launch site of stats.hip takes its block counts, the covariance
// route and configuration, the quantile route and the shape of a lag set from here; the CU count comes in as an argument.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

// Blocks per group (a column, a lag, a column's lag) of the kernels that stride over the rows: `per_cu` blocks per CU
// over all groups, at least `floor`, two per CU at most.
inline int group_blocks(int cu_count, int groups, int floor = 8, int per_cu = 8) {
    int nblk = (per_cu * cu_count + groups - 1) / groups;
    if (nblk < floor) nblk = floor;
    if (nblk > 2 * cu_count) nblk = 2 * cu_count;
    return nblk;
}

// `want` chunks of the rows, each of at least `min_rows` rows (one chunk at least) and a multiple of `quantum` rows;
// n = the chunks that then hold rows.
struct RowChunks { int n; int64_t rows_per_chunk; };
inline RowChunks row_chunks(int64_t rows, int want, int min_rows, int quantum) {
    RowChunks r = {want, 0};
    if (r.n > (rows + min_rows - 1) / min_rows) r.n = (int)((rows + min_rows - 1) / min_rows);
    if (r.n < 1) r.n = 1;
    r.rows_per_chunk = (rows + r.n - 1) / r.n;
    r.rows_per_chunk = (r.rows_per_chunk + quantum - 1) / quantum * quantum;
    r.n = (int)((rows + r.rows_per_chunk - 1) / r.rows_per_chunk);
    return r;
}

// ---- covariance ------------------------------------------------------------------------------------------------------------
// The slab kernel k_cov_slab2<HAS_W, MCAP, NW, NH, P, KS, DEPTH, OP> holds all m columns of a slab of KS rows in LDS: NW
// waves in NH row-splits, P tile pairs of 16 x 16 per wave; bpc = blocks per CU its registers and LDS leave.  This table is
// both what the plan picks from and what the dispatch instantiates.
struct CovCfg { int mcap, nw, nh, p, bpc; };
constexpr CovCfg COV_CFGS[] = {{64, 8, 8, 3, 4},  {64, 8, 4, 3, 4},   {64, 8, 4, 5, 4},   {112, 8, 2, 4, 2}, {112, 8, 2, 6, 2},
                               {112, 8, 2, 7, 2}, {208, 16, 2, 6, 1}, {208, 16, 1, 5, 1}, {208, 16, 1, 6, 1}};
constexpr int COV_NCFG = (int)(sizeof(COV_CFGS) / sizeof(COV_CFGS[0]));
constexpr int COV_SLAB_MAX = 208;                                  // wider matrices take the tile kernel
constexpr int cov_ks(int mc) { return mc <= 64 ? 64 : 32; }        // narrow matrices: more rows per barrier pair
constexpr int cov_depth(int mc) { return mc <= 64 ? 2 : 1; }
#define CT 64   // the tile kernel k_cov_tile: one block = one CT x CT tile of column pairs over one chunk of rows,
#define CRB 64  // which it reads CRB rows at a time

enum CovRoute { COV_ONEPASS, COV_TWOPASS, COV_TILE };
struct CovSlabPlan {
    CovRoute route;  // COV_TILE: nothing below is set
    int me;          // columns in LDS: m, and the ones column of the one-pass form
    int nt16, T, mc, KS;
    int pick;        // index into COV_CFGS, -1: none fits
    size_t lds;      // dynamic LDS bytes of a block
    int bpc, nblk;
    int64_t rows_per_chunk;
};
// One pass: no means pass in front -- a provisional shift, the ones column, k_cov_onepass_fin.  m = COV_SLAB_MAX has no
// room for the extra column and keeps the two passes.
inline CovSlabPlan cov_slab_plan(int m, int64_t rows, int cu_count, bool weighted, bool twopass_forced) {
    CovSlabPlan p = {};
    p.pick = -1;
    const bool onepass = m + 1 <= COV_SLAB_MAX && !twopass_forced;
    p.route = m > COV_SLAB_MAX ? COV_TILE : onepass ? COV_ONEPASS : COV_TWOPASS;
    if (p.route == COV_TILE) return p;
    p.me = onepass ? m + 1 : m;
    p.nt16 = (p.me + 15) / 16, p.T = p.nt16 * (p.nt16 + 1) / 2, p.mc = p.nt16 * 16;
    p.KS = cov_ks(p.mc);
    // the wave arrangement with the fewest tile-pair slots >= T
    for (int k = 0; k < COV_NCFG && p.pick < 0; ++k)
        if (COV_CFGS[k].mcap >= p.mc && (COV_CFGS[k].nw / COV_CFGS[k].nh) * COV_CFGS[k].p >= p.T) p.pick = k;
    if (p.pick < 0) return p;
    const CovCfg cf = COV_CFGS[p.pick];
    p.lds = (size_t)(weighted ? 2 : 1) * p.mc * (p.KS + 2) * 8 + (onepass ? (size_t)p.mc * 8 : 0);
    const size_t split_sum = (size_t)(cf.nw / cf.nh) * cf.p * 256 * 8;  // the in-block sum over the row-splits
    if (cf.nh > 1 && p.lds < split_sum) p.lds = split_sum;
    p.bpc = cf.bpc;
    while (p.bpc > 1 && (size_t)p.bpc * p.lds > 150u * 1024u) --p.bpc;
    const RowChunks rc = row_chunks(rows, p.bpc * cu_count, 4 * p.KS, p.KS);
    p.nblk = rc.n, p.rows_per_chunk = rc.rows_per_chunk;
    return p;
}

struct CovTile { int a, b; };  // (the kernels read it as an int2)
struct CovTilePlan {
    std::vector<CovTile> tiles;  // the upper triangle of CT x CT tiles, row by row
    int nchunks;
    int64_t rows_per_chunk;
};
inline CovTilePlan cov_tile_plan(int m, int64_t rows, int cu_count) {
    CovTilePlan p;
    const int nt = (m + CT - 1) / CT;
    for (int a = 0; a < nt; ++a)
        for (int b = a; b < nt; ++b) p.tiles.push_back(CovTile{a, b});
    const int ntp = (int)p.tiles.size();
    const RowChunks rc = row_chunks(rows, (2 * cu_count + ntp - 1) / ntp, CRB, CRB);
    p.nchunks = rc.n, p.rows_per_chunk = rc.rows_per_chunk;
    return p;
}

// ---- quantile select -------------------------------------------------------------------------------------------------------
#define QLIN_NB_U 32768  // buckets of the linear route's counting pass: unit weights (u32 counters),
#define QLIN_NB_W 16384  // real weights (fp64 sums)

// Blocks per column of the linear route's counting pass: the chip filled about twice over, but every block keeps at least
// 256K rows to spread its 128-KB table's zero-fill and flush over (few columns -- one rank's share of the parameters --
// would otherwise get 64 blocks of 150K rows each).
inline int qlin_count_blocks(int cu_count, int ncols, int64_t rows) {
    int nblk = (2 * cu_count + ncols - 1) / ncols;
    if (nblk > 32) nblk = 32;
    if ((int64_t)nblk * 262144 > rows) nblk = (int)((rows + 262143) / 262144);
    if (nblk < 1) nblk = 1;
    // one block per CU (the table is 128 KB): ncols * nblk blocks run in ceil(blocks / CUs) rounds, so a count just above a
    // multiple of the CU number wastes most of a round (50 columns x 11 blocks = 2.15 rounds took the time of 3; x 10 =
    // 1.95 rounds: 1.40 -> 1.05 ms).  Among the counts down to half of the first choice take the one that fills its
    // rounds best.
    int best = nblk;
    double best_eff = 0;
    for (int q = nblk; q >= (nblk + 1) / 2 && q >= 1; --q) {
        const double rounds = (double)ncols * q / cu_count;
        const double eff = rounds / ceil(rounds);
        if (eff > best_eff + 0.02) best_eff = eff, best = q;
    }
    return best;
}
// Blocks per column of the radix passes and of both routes' collect pass.  Few: every block flushes its private LDS
// histograms with global atomics on the same per-column bins, so the flush cost (and its contention) grows with the count.
inline int qsel_blocks(int cu_count, int ncols) { return group_blocks(cu_count, ncols); }
// radix passes until the live buckets are short enough to collect and sort
inline int qsel_radix_passes(int64_t rows) { return rows <= 15000000 ? 3 : 4; }
// Whether the linear route can serve a call, given minmax[2c], minmax[2c + 1] = column c's range.  The expected length of a
// live bucket's list is rows / buckets times the peak-to-mean density ratio (about 4 for a Gaussian over its sampled
// range): beyond these row counts the lists would overflow.  Weighted bucket sums are fixed-point integers scaled from the
// weights' total, which is known for the uploaded sample weights (any kind: multiplicities or real); auxiliary weights
// (gd_select_weights) have none.
inline bool qlin_eligible(int64_t rows, bool weighted, double w_sum, const double* minmax, int ncols) {
    if (rows > (weighted ? 12000000 : 25000000)) return false;
    if (weighted && !(w_sum > 1e-200 && w_sum < 1e200)) return false;
    for (int c = 0; c < ncols; ++c) {
        const double a = minmax[2 * c], b = minmax[2 * c + 1];
        if (!(b > a) || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite((double)QLIN_NB_U / (b - a))) return false;
    }
    return true;
}

// ---- Gaussian-kernel lag sums ----------------------------------------------------------------------------------------------
#define KDE_LAG_MAX 8  // lags of a column that one launch takes
// The lag set of the N_eff estimate -- five "far" lags from N/2 (4 k >= N), one or two "near" ones below 256 -- takes the
// folded kernel, which reads every sample once: order[] = the far lags, then the near ones, each in the caller's order.
// Any other set (and any set with `fold_allowed` off or N < 4096) keeps the caller's order.  nlags <= KDE_LAG_MAX.
struct LagSet {
    bool folded;
    int nf, nn;
    int order[KDE_LAG_MAX];  // slot l of a partial holds the caller's lag order[l]
};
inline LagSet classify_lags(int64_t N, const int64_t* lags, int nlags, bool fold_allowed = true) {
    LagSet s = {};
    if (N >= 4096 && fold_allowed) {
        int64_t K0 = N, nmax = 0;
        for (int i = 0; i < nlags; ++i)
            if (4 * lags[i] >= N) {
                s.order[s.nf++] = i;
                K0 = lags[i] < K0 ? lags[i] : K0;
            }
        for (int i = 0; i < nlags; ++i)
            if (4 * lags[i] < N) {
                s.order[s.nf + s.nn++] = i;
                nmax = lags[i] > nmax ? lags[i] : nmax;
            }
        s.folded = s.nf == 5 && (s.nn == 1 || s.nn == 2) && 2 * K0 <= N && nmax < 256;
    }
    if (!s.folded)
        for (int i = 0; i < nlags; ++i) s.order[i] = i;
    return s;
}
