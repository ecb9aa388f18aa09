// Host check of getdist_amd/csrc/statsplan.hpp: the header compiles with g++ (no HIP), and its block counts, covariance
// plans, quantile plans and lag-set classification equal the expressions the launch sites of stats.hip used to write out one
// by one -- they are written out again here, literally, as the reference.  Prints one line per failure and a summary; exit
// status 0 = all equal.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include "../../getdist_amd/csrc/statsplan.hpp"

static long long g_checked = 0, g_bad = 0;
#define EXPECT_EQ(what, got, want, ...)                                                           \
    do {                                                                                          \
        ++g_checked;                                                                              \
        if ((long long)(got) != (long long)(want)) {                                              \
            if (++g_bad <= 20) {                                                                  \
                printf("MISMATCH %s: %lld != %lld at ", what, (long long)(got), (long long)(want)); \
                printf(__VA_ARGS__);                                                              \
                printf("\n");                                                                     \
            }                                                                                     \
        }                                                                                         \
    } while (0)

// ---- the former expressions ---------------------------------------------------------------------------------------------
struct OldCov {
    bool slab, onepass;
    int me, nt16, T, mc, KS, pick, bpc, nblk;  // slab
    size_t lds;
    int64_t rows_per_chunk;
    std::vector<std::pair<int, int>> tiles;  // tile
    int nchunks;
};
static OldCov old_cov(int m, int64_t rows, int cu_count, bool hw, bool twopass_env) {
    OldCov o = {};
    const bool slab = (m <= 208);
    o.slab = slab;
    if (slab) {
        const bool onepass = m + 1 <= 208 && !twopass_env;
        const int me = onepass ? m + 1 : m;
        const int nt16 = (me + 15) / 16, T = nt16 * (nt16 + 1) / 2, mc = nt16 * 16;
        const int KS = mc <= 64 ? 64 : 32;
        struct Cfg { int mcap, nw, nh, p, bpc; };
        static const Cfg cfgs[] = {{64, 8, 8, 3, 4},  {64, 8, 4, 3, 4},   {64, 8, 4, 5, 4},   {112, 8, 2, 4, 2}, {112, 8, 2, 6, 2},
                                   {112, 8, 2, 7, 2}, {208, 16, 2, 6, 1}, {208, 16, 1, 5, 1}, {208, 16, 1, 6, 1}};
        int pick = -1;
        for (int k = 0; k < (int)(sizeof(cfgs) / sizeof(cfgs[0])); ++k)
            if (cfgs[k].mcap >= mc && (cfgs[k].nw / cfgs[k].nh) * cfgs[k].p >= T) {
                pick = k;
                break;
            }
        o.onepass = onepass, o.me = me, o.nt16 = nt16, o.T = T, o.mc = mc, o.KS = KS, o.pick = pick;
        if (pick < 0) return o;
        const Cfg cf = cfgs[pick];
        size_t lds = (size_t)(hw ? 2 : 1) * mc * (KS + 2) * 8 + (onepass ? (size_t)mc * 8 : 0);
        if (cf.nh > 1) lds = std::max(lds, (size_t)(cf.nw / cf.nh) * cf.p * 256 * 8);
        int bpc = cf.bpc;
        while (bpc > 1 && (size_t)bpc * lds > 150u * 1024u) --bpc;
        int nblk = bpc * cu_count;
        if (nblk > (rows + 4 * KS - 1) / (4 * KS)) nblk = (int)((rows + 4 * KS - 1) / (4 * KS));
        if (nblk < 1) nblk = 1;
        int64_t rows_per_chunk = (rows + nblk - 1) / nblk;
        rows_per_chunk = (rows_per_chunk + KS - 1) / KS * KS;
        nblk = (int)((rows + rows_per_chunk - 1) / rows_per_chunk);
        o.lds = lds, o.bpc = bpc, o.nblk = nblk, o.rows_per_chunk = rows_per_chunk;
    } else {
        const int nt = (m + 64 - 1) / 64;
        for (int a = 0; a < nt; ++a)
            for (int b = a; b < nt; ++b) o.tiles.push_back(std::make_pair(a, b));
        const int ntp = (int)o.tiles.size();
        int nchunks = (2 * cu_count + ntp - 1) / ntp;
        if (nchunks > (rows + 64 - 1) / 64) nchunks = (int)((rows + 64 - 1) / 64);
        if (nchunks < 1) nchunks = 1;
        int64_t rows_per_chunk = (rows + nchunks - 1) / nchunks;
        rows_per_chunk = (rows_per_chunk + 64 - 1) / 64 * 64;
        nchunks = (int)((rows + rows_per_chunk - 1) / rows_per_chunk);
        o.nchunks = nchunks, o.rows_per_chunk = rows_per_chunk;
    }
    return o;
}
// the template arguments the former dispatch macro gave case `pick`: <MCAP, NW, NH, P, KS, DEPTH>
static const int OLD_SWITCH[9][6] = {{64, 8, 8, 3, 64, 2},  {64, 8, 4, 3, 64, 2},   {64, 8, 4, 5, 64, 2},
                                     {112, 8, 2, 4, 32, 1}, {112, 8, 2, 6, 32, 1},  {112, 8, 2, 7, 32, 1},
                                     {208, 16, 2, 6, 32, 1}, {208, 16, 1, 5, 32, 1}, {208, 16, 1, 6, 32, 1}};

static int old_clamp(int cu_count, int items, int floor) {
    int nblk = (8 * cu_count + items - 1) / items;
    if (nblk < floor) nblk = floor;
    if (nblk > 2 * cu_count) nblk = 2 * cu_count;
    return nblk;
}
static int old_qlin_blocks(int cu_count, int ncols, int64_t lo, int64_t hi) {
    int nblk = (2 * cu_count + ncols - 1) / ncols;
    if (nblk > 32) nblk = 32;
    if ((int64_t)nblk * 262144 > hi - lo) nblk = (int)((hi - lo + 262143) / 262144);
    if (nblk < 1) nblk = 1;
    {
        int best = nblk;
        double best_eff = 0;
        for (int q = nblk; q >= (nblk + 1) / 2 && q >= 1; --q) {
            const double rounds = (double)ncols * q / cu_count;
            const double eff = rounds / ceil(rounds);
            if (eff > best_eff + 0.02) best_eff = eff, best = q;
        }
        nblk = best;
    }
    return nblk;
}
static bool old_linear(int64_t lo, int64_t hi, bool has_w, double w_sum, const double* minmax, int ncols) {
    bool linear = true;
    if (linear && (hi - lo) > (has_w ? 12000000 : 25000000)) linear = false;
    if (linear && has_w && !(w_sum > 1e-200 && w_sum < 1e200)) linear = false;
    for (int c = 0; linear && c < ncols; ++c) {
        const double a = minmax[2 * c], b = minmax[2 * c + 1];
        if (!(b > a) || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite((double)32768 / (b - a))) linear = false;
    }
    return linear;
}
struct OldLags {
    bool folded;
    int nf, nn;
    int order[8];
};
static OldLags old_lags(int64_t N, const int64_t* lags, int nlags, bool unfolded_env) {
    OldLags o = {};
    int* order = o.order;
    int nf = 0, nn = 0;
    bool folded = false;
    if (N >= 4096 && !unfolded_env) {
        int64_t K0 = N, nmax = 0;
        for (int i = 0; i < nlags; ++i)
            if (4 * lags[i] >= N) {
                order[nf++] = i;
                K0 = lags[i] < K0 ? lags[i] : K0;
            }
        for (int i = 0; i < nlags; ++i)
            if (4 * lags[i] < N) {
                order[nf + nn++] = i;
                nmax = lags[i] > nmax ? lags[i] : nmax;
            }
        folded = nf == 5 && (nn == 1 || nn == 2) && 2 * K0 <= N && nmax < 256;
    }
    if (!folded)
        for (int i = 0; i < nlags && i < 8; ++i) order[i] = i;
    o.folded = folded, o.nf = nf, o.nn = nn;
    return o;
}

static void check_lags(int64_t N, const int64_t* lags, int nlags, int want_folded) {
    for (int unfolded = 0; unfolded < 2; ++unfolded) {
        const OldLags o = old_lags(N, lags, nlags, unfolded != 0);
        const LagSet s = classify_lags(N, lags, nlags, !unfolded);
        EXPECT_EQ("lag set folded", s.folded, o.folded, "N %lld nlags %d", (long long)N, nlags);
        EXPECT_EQ("lag set nf", s.nf, o.nf, "N %lld nlags %d", (long long)N, nlags);
        EXPECT_EQ("lag set nn", s.nn, o.nn, "N %lld nlags %d", (long long)N, nlags);
        EXPECT_EQ("lag set order", memcmp(s.order, o.order, sizeof(int) * nlags), 0, "N %lld nlags %d", (long long)N, nlags);
        if (want_folded >= 0) EXPECT_EQ("lag set takes the expected kernel", s.folded, unfolded ? 0 : want_folded, "N %lld", (long long)N);
    }
}

int main() {
    static_assert(COV_NCFG == 9 && COV_SLAB_MAX == 208 && CT == 64 && CRB == 64, "the kernels are written for these");
    static_assert(QLIN_NB_U == 32768 && QLIN_NB_W == 16384 && KDE_LAG_MAX == 8, "the kernels are written for these");
    // the table against what the former dispatch instantiated, case by case
    for (int k = 0; k < COV_NCFG; ++k) {
        const CovCfg c = COV_CFGS[k];
        const int got[6] = {c.mcap, c.nw, c.nh, c.p, cov_ks(c.mcap), cov_depth(c.mcap)};
        for (int j = 0; j < 6; ++j) EXPECT_EQ("dispatch template argument", got[j], OLD_SWITCH[k][j], "cfg %d arg %d", k, j);
    }

    // ---- covariance: m x rows x CU x weighted x two-pass forced
    const int64_t cov_rows[] = {1, 63, 64, 257, 3000, 1000000, 10000000};
    const int cus[] = {64, 256, 304};
    int first_m[9];
    for (int k = 0; k < 9; ++k) first_m[k] = -1;
    for (int m = 1; m <= 260; ++m)
        for (int64_t rows : cov_rows)
            for (int cu : cus)
                for (int hw = 0; hw < 2; ++hw)
                    for (int two = 0; two < 2; ++two) {
                        const OldCov o = old_cov(m, rows, cu, hw, two);
                        const CovSlabPlan p = cov_slab_plan(m, rows, cu, hw, two);
#define AT "m %d rows %lld cu %d hw %d twopass %d", m, (long long)rows, cu, hw, two
                        EXPECT_EQ("slab route", p.route != COV_TILE, o.slab, AT);
                        if (o.slab) {
                            EXPECT_EQ("one pass", p.route == COV_ONEPASS, o.onepass, AT);
                            EXPECT_EQ("me", p.me, o.me, AT);
                            EXPECT_EQ("nt16", p.nt16, o.nt16, AT);
                            EXPECT_EQ("T", p.T, o.T, AT);
                            EXPECT_EQ("mc", p.mc, o.mc, AT);
                            EXPECT_EQ("KS", p.KS, o.KS, AT);
                            EXPECT_EQ("pick", p.pick, o.pick, AT);
                            EXPECT_EQ("a configuration fits", p.pick >= 0, 1, AT);
                            if (p.pick < 0 || o.pick < 0) continue;
                            // the kernel's own KS (from its MCAP) is the plan's (from mc), and the matrix fits its slab
                            EXPECT_EQ("kernel KS", cov_ks(COV_CFGS[p.pick].mcap), p.KS, AT);
                            EXPECT_EQ("mc <= MCAP", p.mc <= COV_CFGS[p.pick].mcap, 1, AT);
                            EXPECT_EQ("lds", p.lds, o.lds, AT);
                            EXPECT_EQ("bpc", p.bpc, o.bpc, AT);
                            EXPECT_EQ("nblk", p.nblk, o.nblk, AT);
                            EXPECT_EQ("rows_per_chunk", p.rows_per_chunk, o.rows_per_chunk, AT);
                            EXPECT_EQ("blocks cover the rows", (int64_t)p.nblk * p.rows_per_chunk >= rows, 1, AT);
                            if (!two && p.route == COV_ONEPASS && first_m[p.pick] < 0) first_m[p.pick] = m;
                        } else {
                            const CovTilePlan t = cov_tile_plan(m, rows, cu);
                            EXPECT_EQ("tiles", t.tiles.size(), o.tiles.size(), AT);
                            for (size_t i = 0; i < t.tiles.size() && i < o.tiles.size(); ++i) {
                                EXPECT_EQ("tile a", t.tiles[i].a, o.tiles[i].first, AT);
                                EXPECT_EQ("tile b", t.tiles[i].b, o.tiles[i].second, AT);
                            }
                            EXPECT_EQ("nchunks", t.nchunks, o.nchunks, AT);
                            EXPECT_EQ("tile rows_per_chunk", t.rows_per_chunk, o.rows_per_chunk, AT);
                            EXPECT_EQ("chunks cover the rows", (int64_t)t.nchunks * t.rows_per_chunk >= rows, 1, AT);
                        }
#undef AT
                    }
    // the configuration boundaries
    const int want_first[9] = {1, 32, 48, 64, 80, 96, 112, 144, 192};
    for (int k = 0; k < 9; ++k) EXPECT_EQ("first m of a one-pass configuration", first_m[k], want_first[k], "cfg %d", k);
    for (int m = 1; m <= 260; ++m) {
        const CovSlabPlan p = cov_slab_plan(m, 3000, 256, false, false);
        EXPECT_EQ("route", p.route, m <= 207 ? COV_ONEPASS : m == 208 ? COV_TWOPASS : COV_TILE, "m %d", m);
    }
    EXPECT_EQ("m = 208 takes configuration 8", cov_slab_plan(208, 3000, 256, true, false).pick, 8, "weighted");
    EXPECT_EQ("four tiles from m = 209 on", cov_tile_plan(209, 3000, 256).tiles.size(), 10, "tile pairs of a 4 x 4 triangle");

    // ---- block counts: the five former clamps and the linear route's counting pass
    const int64_t q_rows[] = {1000, 262144, 262145, 10000000, 25000000};
    for (int cu : {1, 3, 64, 256, 304})
        for (int items = 1; items <= 64; ++items) {
            EXPECT_EQ("group_blocks floor 8", group_blocks(cu, items), old_clamp(cu, items, 8), "cu %d items %d", cu, items);
            EXPECT_EQ("group_blocks floor 16", group_blocks(cu, items, 16), old_clamp(cu, items, 16), "cu %d items %d", cu, items);
            EXPECT_EQ("qsel_blocks", qsel_blocks(cu, items), old_clamp(cu, items, 8), "cu %d ncols %d", cu, items);
            for (int nlags : {9, 64})  // the single-lag kernel: ncols x nlags groups
                EXPECT_EQ("group_blocks(ncols x nlags)", group_blocks(cu, items * nlags), old_clamp(cu, items * nlags, 8), "cu %d", cu);
            for (int64_t rows : q_rows)
                for (int64_t lo : {(int64_t)0, (int64_t)17})
                    EXPECT_EQ("qlin_count_blocks", qlin_count_blocks(cu, items, rows), old_qlin_blocks(cu, items, lo, lo + rows),
                              "cu %d ncols %d rows %lld", cu, items, (long long)rows);
        }
    for (int64_t rows : {(int64_t)1, (int64_t)14999999, (int64_t)15000000, (int64_t)15000001, (int64_t)25000000})
        EXPECT_EQ("radix passes", qsel_radix_passes(rows), rows <= 15000000 ? 3 : 4, "rows %lld", (long long)rows);

    // ---- the linear route's eligibility
    {
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        const double w_sums[] = {0, 1e-201, 1e-200, 1, 1e200, 1e201, inf, nan, -1};
        const double bounds[][2] = {{0, 1},     {-3, 3},    {1, 1},        {2, 1},       {-inf, 1},       {0, inf},
                                    {nan, 1},   {0, nan},   {0, 1e-310},   {0, 4e-304},  {1, 1 + 1e-15},  {-1e308, 1e308},
                                    {0, 5e-324}};
        const int nbounds = (int)(sizeof(bounds) / sizeof(bounds[0]));
        const int64_t caps[] = {1, 11999999, 12000000, 12000001, 24999999, 25000000, 25000001};
        long long eligible = 0;
        for (int64_t rows : caps)
            for (int hw = 0; hw < 2; ++hw)
                for (double w_sum : w_sums)
                    for (int i = 0; i < nbounds; ++i)
                        for (int j = 0; j < nbounds; ++j) {
                            const double mm[4] = {bounds[i][0], bounds[i][1], bounds[j][0], bounds[j][1]};
                            for (int ncols = 1; ncols <= 2; ++ncols) {
                                const bool want = old_linear(5, 5 + rows, hw, w_sum, mm, ncols);
                                EXPECT_EQ("qlin_eligible", qlin_eligible(rows, hw, w_sum, mm, ncols), want,
                                          "rows %lld hw %d w_sum %g bounds %d %d ncols %d", (long long)rows, hw, w_sum, i, j, ncols);
                                eligible += want;
                            }
                        }
        EXPECT_EQ("some calls are eligible", eligible > 0, 1, "eligibility sweep");
        const double ok[2] = {0, 1}, tiny[2] = {0, 1e-310};
        EXPECT_EQ("unit weights at the cap", qlin_eligible(25000000, false, nan, ok, 1), 1, "25e6 rows");
        EXPECT_EQ("unit weights past the cap", qlin_eligible(25000001, false, 1, ok, 1), 0, "25e6 + 1 rows");
        EXPECT_EQ("real weights at the cap", qlin_eligible(12000000, true, 1, ok, 1), 1, "12e6 rows");
        EXPECT_EQ("real weights past the cap", qlin_eligible(12000001, true, 1, ok, 1), 0, "12e6 + 1 rows");
        EXPECT_EQ("no weight total", qlin_eligible(1000, true, 0, ok, 1), 0, "w_sum 0");
        EXPECT_EQ("the scale overflows", qlin_eligible(1000, false, 1, tiny, 1), 0, "b - a = 1e-310");
    }

    // ---- lag sets
    {
        std::mt19937_64 rng(20240611);
        const int64_t Ns[] = {4095, 4096, 4097, 50001};
        long long folded = 0;
        for (int t = 0; t < 10000; ++t) {
            const int64_t N = Ns[t % 4];
            int64_t lags[8];
            int nlags;
            if (t % 2) {  // near the N_eff shape: about five far lags from about N / 2, about one or two near ones, shuffled
                const int nf = 4 + (int)(rng() % 3), nn = (int)(rng() % 4);
                nlags = 0;
                const int64_t K0 = N / 2 - 1 + (int64_t)(rng() % 3);
                for (int i = 0; i < nf && nlags < 8; ++i) lags[nlags++] = std::min(N - 1, K0 + (int64_t)(rng() % 6));
                for (int i = 0; i < nn && nlags < 8; ++i) lags[nlags++] = 1 + (int64_t)(rng() % 258);
                std::shuffle(lags, lags + nlags, rng);
            } else {
                nlags = 1 + (int)(rng() % 8);
                for (int i = 0; i < nlags; ++i) lags[i] = 1 + (int64_t)(rng() % (N - 1));
            }
            folded += classify_lags(N, lags, nlags).folded;
            check_lags(N, lags, nlags, -1);
        }
        EXPECT_EQ("the random lists reach both kernels", folded > 100 && folded < 9900, 1, "folded %lld of 10000", folded);
        for (int64_t N : {(int64_t)4096, (int64_t)4097, (int64_t)50000, (int64_t)50001, (int64_t)131075}) {
            const int64_t h = N / 2;
            // the three orderings of the GPU test of the folded kernel
            const int64_t a[] = {h, h + 1, h + 2, h + 3, h + 4, 1, 2}, b[] = {h, h + 1, h + 2, h + 3, h + 4, 1};
            const int64_t c[] = {1, 2, h + 4, h, h + 2, h + 1, h + 3};
            check_lags(N, a, 7, 1), check_lags(N, b, 6, 1), check_lags(N, c, 7, 1);
            const LagSet s = classify_lags(N, c, 7);
            const int want[7] = {2, 3, 4, 5, 6, 0, 1};
            EXPECT_EQ("far lags first, each kind in the caller's order", memcmp(s.order, want, sizeof want), 0, "N %lld", (long long)N);
            // sets that just miss
            const int64_t four[] = {h, h + 1, h + 2, h + 3, 1, 2}, six[] = {h, h + 1, h + 2, h + 3, h + 4, h + 5, 1};
            const int64_t three[] = {h, h + 1, h + 2, h + 3, h + 4, 1, 2, 3}, none[] = {h, h + 1, h + 2, h + 3, h + 4};
            const int64_t n256[] = {h, h + 1, h + 2, h + 3, h + 4, 1, 256}, n255[] = {h, h + 1, h + 2, h + 3, h + 4, 1, 255};
            check_lags(N, four, 6, 0), check_lags(N, six, 7, 0), check_lags(N, three, 8, 0), check_lags(N, none, 5, 0);
            check_lags(N, n256, 7, 0), check_lags(N, n255, 7, 1);
            // 2 * K0 = N + 1 (odd N) or N + 2 (even N): the halves would not cover the rows
            const int64_t k = (N + 2) / 2;
            const int64_t late[] = {k, k + 1, k + 2, k + 3, k + 4, 1, 2};
            check_lags(N, late, 7, 0);
        }
        const int64_t small[] = {2047, 2048, 2049, 2050, 2051, 1, 2};
        check_lags(4095, small, 7, 0);  // below 4096 rows the general kernel
    }
    printf("checked %lld mismatches %lld\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
