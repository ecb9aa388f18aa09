// Host check of getdist_amd/csrc/binplan.hpp: the header compiles with g++ (no HIP), and its stripe geometry, chunk counts,
// block counts, grid sizes and min / max column grouping equal the expressions the launch sites of binning.hip used to write
// out one by one -- they are written out again here, literally, as the reference.  Prints one line per failure and a
// summary; exit status 0 = all equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "../../getdist_amd/csrc/binplan.hpp"

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
static int old_pick_chunks(int cu_count, int64_t units, int64_t rows) {
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
static int old_u8_chunks(int cu_count, int B, int64_t N) {
    if (B >= 2 * cu_count) return 1;
    return old_pick_chunks(cu_count, B, N);
}

struct OldGroups {
    std::vector<MinmaxGroup> groups;
    std::vector<std::vector<int>> members;
};
static void old_minmax_groups(int B, const int32_t* coli, const int32_t* colj, const double* a, const double* b, const double* cols,
                              int64_t ld, OldGroups& O) {
    std::vector<MinmaxGroup>& groups = O.groups;
    std::vector<std::vector<int>>& members = O.members;
    std::vector<int> order((size_t)B);
    for (int q = 0; q < B; ++q) order[q] = q;
    std::sort(order.begin(), order.end(), [&](int u, int v) {
        const int ul = std::min(coli[u], colj[u]), uh = std::max(coli[u], colj[u]);
        const int vl = std::min(coli[v], colj[v]), vh = std::max(coli[v], colj[v]);
        return ul != vl ? ul < vl : (uh != vh ? uh < vh : u < v);
    });
    std::vector<int> gcols;
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
            open = (int)gcols.size() + need <= 8 && groups.back().npairs < 16;
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

int main() {
    static_assert(LDS_HIST_BYTES == 128 * 1024 && MMG_COLS == 8 && MMG_PAIRS == 16, "the kernels are written for these");
    const int Fs[] = {2, 64, 255, 256, 257, 384, 768, 960, 4096};
    const int bytes[] = {2, 4, 8};
    const int Bs[] = {1, 2, 7, 125, 294, 511, 512, 1225};
    const int64_t Ns[] = {1, 65535, 131071, 131072, 200003, 10000000};
    const int cus[] = {256, 64};
    for (int cu : cus) {
        for (int64_t N : Ns) {
            int nblk = (int)((N / 8 + 255) / 256);
            if (nblk > 2 * cu) nblk = 2 * cu;
            if (nblk < 1) nblk = 1;
            EXPECT_EQ("prebin_blocks", prebin_blocks(cu, N), nblk, "cu %d N %lld", cu, (long long)N);
        }
        for (int B : Bs) {
            for (int per_cu : {4, 6}) {
                int nblk = (per_cu * cu + B - 1) / B;
                if (nblk < 8) nblk = 8;
                if (nblk > 1024) nblk = 1024;
                EXPECT_EQ("minmax_blocks", minmax_blocks(cu, per_cu, B), nblk, "cu %d B %d per_cu %d", cu, B, per_cu);
            }
            for (int64_t N : Ns) {
                const int nchunks8 = old_u8_chunks(cu, B, N);
                EXPECT_EQ("u8_chunks", u8_chunks(cu, B, N), nchunks8, "cu %d B %d N %lld", cu, B, (long long)N);
                EXPECT_EQ("byte blocks", unit_blocks(B, nchunks8), (B * nchunks8 + 7) / 8 * 8, "cu %d B %d N %lld", cu, B, (long long)N);
                for (int F : Fs)
                    for (int cb : bytes) {
                        int R = LDS_HIST_BYTES / (F * cb);
                        if (R > F) R = F;
                        const int nstripes = (F + R - 1) / R;
                        const int nwords = (R * F + 1) / 2;
                        const int nchunks = old_pick_chunks(cu, (int64_t)B * nstripes, N);
                        const int units = (B * nchunks + 7) / 8 * 8;
                        const int64_t nblocks = (int64_t)units * nstripes;
                        const StripeGeom g = stripe_geom(F, cb);
                        EXPECT_EQ("R", g.R, R, "F %d bytes %d", F, cb);
                        EXPECT_EQ("nstripes", g.nstripes, nstripes, "F %d bytes %d", F, cb);
                        EXPECT_EQ("nwords", g.nwords, nwords, "F %d bytes %d", F, cb);
                        const int got = pick_chunks(cu, (int64_t)B * g.nstripes, N);
                        EXPECT_EQ("pick_chunks", got, nchunks, "cu %d B %d N %lld F %d bytes %d", cu, B, (long long)N, F, cb);
                        EXPECT_EQ("unit_blocks", unit_blocks(B, got, g.nstripes), nblocks, "cu %d B %d N %lld F %d bytes %d", cu, B,
                                  (long long)N, F, cb);
                        // the one-block-per-(pair, stripe) launch
                        EXPECT_EQ("unit_blocks(1 chunk)", unit_blocks(B, 1, g.nstripes), (int64_t)((B + 7) / 8 * 8) * nstripes,
                                  "B %d F %d bytes %d", B, F, cb);
                    }
            }
        }
    }
    // the wrap test of tests/test_gpu_primitives.py relies on this: three chunks for two pairs of 200 003 rows on 256 CUs
    EXPECT_EQ("pick_chunks(256, 2 x 2 stripes, 200003)", pick_chunks(256, 2 * stripe_geom(384, 2).nstripes, 200003), 3, "F 384");
    EXPECT_EQ("pick_chunks(256, 2 x 1 stripe, 200003)", pick_chunks(256, 2 * stripe_geom(256, 2).nstripes, 200003), 3, "F 256");

    // min / max grouping: 1000 random pair lists over <= 12 columns
    static double storage[12 * 3];
    const int64_t ld = 3;
    std::mt19937 rng(12345);
    for (int t = 0; t < 1000; ++t) {
        const int ncols = 1 + (int)(rng() % 12), B = 1 + (int)(rng() % 70);
        std::vector<int32_t> ci((size_t)B), cj((size_t)B);
        std::vector<double> a((size_t)B), b((size_t)B);
        for (int q = 0; q < B; ++q) {
            ci[q] = (int32_t)(rng() % ncols), cj[q] = (int32_t)(rng() % ncols);  // (i, i) pairs included
            a[q] = (double)(rng() % 1000) / 7.0, b[q] = -(double)(rng() % 1000) / 3.0;
        }
        OldGroups O;
        old_minmax_groups(B, ci.data(), cj.data(), a.data(), b.data(), storage, ld, O);
        std::vector<MinmaxGroup> groups;
        std::vector<std::vector<int>> members;
        minmax_groups(B, ci.data(), cj.data(), a.data(), b.data(), storage, ld, groups, members);
        EXPECT_EQ("groups", groups.size(), O.groups.size(), "list %d", t);
        EXPECT_EQ("member lists", members.size(), O.members.size(), "list %d", t);
        if (groups.size() != O.groups.size() || members.size() != O.members.size()) continue;
        for (size_t g = 0; g < groups.size(); ++g) {
            // whole records, bit for bit: column pointers, coefficients, slots, counts (both were zero-filled first)
            EXPECT_EQ("group record", memcmp(&groups[g], &O.groups[g], sizeof(MinmaxGroup)), 0, "list %d group %d", t, (int)g);
            EXPECT_EQ("member order", members[g] == O.members[g], 1, "list %d group %d", t, (int)g);
            EXPECT_EQ("members per group", (int)members[g].size(), groups[g].npairs, "list %d group %d", t, (int)g);
        }
    }
    printf("checked %lld mismatches %lld\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
