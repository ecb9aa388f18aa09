// The launch arithmetic of binning.hip in one place (plain C++17, no HIP: compiles with g++ like scratchplan.hpp;
// tests/native/binplan_check.cpp sweeps it).  Every launch site of binning.hip takes its stripe geometry, chunk count,
// block count and grid size from here; the CU count comes in as an argument.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define LDS_HIST_BYTES (128 * 1024)  // the counter table of one workgroup

// A workgroup owns a stripe of R rows of the F x F grid (R * F counters <= LDS_HIST_BYTES); nwords = the stripe's packed
// 16-bit counters in 32-bit words.  R = 0: one row does not fit.
struct StripeGeom {
    int R, nstripes, nwords;
};
inline StripeGeom stripe_geom(int F, int counter_bytes) {
    StripeGeom g;
    g.R = LDS_HIST_BYTES / (F * counter_bytes);
    if (g.R > F) g.R = F;
    g.nstripes = g.R > 0 ? (F + g.R - 1) / g.R : 0;
    g.nwords = (g.R * F + 1) / 2;
    return g;
}

// How many row chunks to cut every (pair, stripe) unit into.  The 128-KB counter table leaves one block per CU, so a
// launch runs in ceil(blocks / CUs) rounds of one block time each, and a block's time is proportional to its rows:
// the cost of c chunks is rounds(c) / c.  (The old rule, "at least two blocks per CU", gave 79 sheared pairs 553
// blocks = 2.16 -> three rounds of N/7 rows; three chunks give one round of N/3.)  A small penalty per chunk accounts
// for the zero-fill, flush and reduction of its partial table; at most 16 chunks.
inline int pick_chunks(int cu_count, int64_t units, int64_t rows) {
    int best = 1;
    double best_cost = 1e30;
    for (int c = 1; c <= 16; ++c) {
        if ((int64_t)c * 65536 > rows && c > 1) break;
        const int64_t blocks = units * c;
        const double rounds = (double)((blocks + cu_count - 1) / cu_count);
        const double cost = rounds / c + 0.004 * c;
        if (cost < best_cost - 1e-12) best_cost = cost, best = c;
    }
    return best;
}
// chunks per pair of the byte-index launch: none for a whole triangle (the partial tables would cost more than the round
// quantisation), else what fills the rounds
inline int u8_chunks(int cu_count, int B, int64_t N) {
    if (B >= 2 * cu_count) return 1;
    return pick_chunks(cu_count, B, N);
}
// blocks of a launch over (pair, chunk) units: whole groups of eight units (block id mod 8 = XCD), `nstripes` blocks each
inline int64_t unit_blocks(int B, int nchunks, int nstripes = 1) {
    const int units = (B * nchunks + 7) / 8 * 8;
    return (int64_t)units * nstripes;
}
// blocks per column of the fp64 pre-bin kernels: one 8-sample iteration per thread at most, two blocks per CU at most
inline int prebin_blocks(int cu_count, int64_t N) {
    int nblk = (int)((N / 8 + 255) / 256);
    if (nblk > 2 * cu_count) nblk = 2 * cu_count;
    if (nblk < 1) nblk = 1;
    return nblk;
}
// blocks per unit (pair or group) of the min / max kernels: `per_cu` blocks per CU over all units, 8..1024
inline int minmax_blocks(int cu_count, int per_cu, int units) {
    int nblk = (per_cu * cu_count + units - 1) / units;
    if (nblk < 8) nblk = 8;
    if (nblk > 1024) nblk = 1024;
    return nblk;
}

// Several sheared pairs share their columns (a correlated block of 5 parameters gives 10 pairs over 5 columns): a group
// of <= 16 pairs over <= 8 distinct columns reads each column ONCE (k_minmax_affine_grouped).
#define MMG_COLS 8
#define MMG_PAIRS 16
struct MinmaxGroup {
    const double* col[MMG_COLS];
    double r0[MMG_PAIRS], r1[MMG_PAIRS];
    int a[MMG_PAIRS], b[MMG_PAIRS];
    int ncols, npairs;
};
// The pairs (coli[q], colj[q]) with coefficients (a[q], b[q]) in groups over shared columns, in the order of their
// (lower, higher) column; members[g][p] = the pair that slot p of group g serves.  Column c starts at cols + c * ld.
inline void minmax_groups(int B, const int32_t* coli, const int32_t* colj, const double* a, const double* b, const double* cols,
                          int64_t ld, std::vector<MinmaxGroup>& groups, std::vector<std::vector<int>>& members) {
    std::vector<int> order((size_t)B);
    for (int q = 0; q < B; ++q) order[q] = q;
    std::sort(order.begin(), order.end(), [&](int u, int v) {
        const int ul = std::min(coli[u], colj[u]), uh = std::max(coli[u], colj[u]);
        const int vl = std::min(coli[v], colj[v]), vh = std::max(coli[v], colj[v]);
        return ul != vl ? ul < vl : (uh != vh ? uh < vh : u < v);
    });
    std::vector<int> gcols;  // column ids of the open group
    auto slot_of = [&](int c) {
        for (size_t k = 0; k < gcols.size(); ++k)
            if (gcols[k] == c) return (int)k;
        return -1;
    };
    for (int q : order) {
        const int ci = coli[q], cj = colj[q];
        bool open = !groups.empty();
        if (open) {
            const int need = (slot_of(ci) < 0) + (cj != ci && slot_of(cj) < 0);
            open = (int)gcols.size() + need <= MMG_COLS && groups.back().npairs < MMG_PAIRS;
        }
        if (!open) {
            MinmaxGroup g;
            memset(&g, 0, sizeof g);
            groups.push_back(g);
            members.emplace_back();
            gcols.clear();
        }
        MinmaxGroup& g = groups.back();
        for (int c : {ci, cj})
            if (slot_of(c) < 0) {
                g.col[gcols.size()] = cols + (int64_t)c * ld;
                gcols.push_back(c);
            }
        g.ncols = (int)gcols.size();
        g.a[g.npairs] = slot_of(ci), g.b[g.npairs] = slot_of(cj);
        g.r0[g.npairs] = a[q], g.r1[g.npairs] = b[q];
        members.back().push_back(q);
        ++g.npairs;
    }
}
