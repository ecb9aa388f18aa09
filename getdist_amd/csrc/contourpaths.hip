// Contour paths of a batch of 2D grids: for every (grid, level) the boundary of {P > level} as closed, ordered loops
// (what matplotlib's ax.contour / ax.contourf get from contourpy on the host, one grid at a time).
//
// The grid is surrounded by one ring of virtual nodes that are always below the level and sit on the edge nodes, so
// every contour is a closed loop: where {P > level} touches the domain edge the loop runs along the edge (those
// vertices carry flag 1).  Edges of the padded (ny+2) x (nx+2) lattice are numbered: horizontal (j,i)-(j,i+1) has id
// j*(nx+1)+i, vertical (j,i)-(j+1,i) has id (ny+2)*(nx+1) + j*(nx+2)+i.  An edge is crossed when exactly one end is
// above; a crossed edge carries one vertex, starts one segment (in the cell that has the above end first on its
// counter-clockwise walk) and ends one, so the segments form disjoint cycles with the above side on the left.
// The canonical order lists the cycles by their smallest edge id, each from that edge on.
//
// One workgroup per (grid, level) task:
//   k_cp_count   counts the task's crossed edges (a wave ballots 64 consecutive edge ids per step) and leaves the bitmap of
//                crossed edges with its per-word counts; the counts are scanned (tilescan.hpp) and only the totals come
//                back, so results and scratch are sized exactly;
//   k_cp_paths   scans the per-word counts (slot of an edge in O(1): prefix[word] + popcount of the lower bits), compacts
//                the crossed edges in id order with the slot of the edge their segment ends on, and orders the cycles by
//                pointer jumping: ceil(log2 n) rounds of minimum propagation give every slot its cycle's leader (smallest
//                slot = smallest id), the cycle is cut in front of the leader and ceil(log2 n) rounds of list ranking give
//                the distance to the cut; a scan over the leaders (already in id order) numbers the loops and places
//                them, and every vertex goes to loop base + rank.  All rounds read one table and write the other, with a
//                barrier between.
// The link tables (CP_SLOT_BYTES per crossed edge) live in LDS while n <= CP_LDS_SLOTS, else in the task's slice of global
// scratch; the code is the same.  Workgroups are handed out largest task first (a triangle has a few grids of 960 x 960
// among 1200 of 256 x 256).  No inter-workgroup dependence, no atomics.
#include "ctx.hpp"
#include "tilescan.hpp"

#include <algorithm>
#include <cmath>

#define CP_THREADS 1024
#define CP_WAVES (CP_THREADS / WAVE)
#define CP_MAXC 8
#define CP_MAX_SIDE 4096
#define CP_LDS_SLOTS 2560  // 70 KB of tables: two workgroups of 1024 threads fill a CU's wave slots and fit its 160 KB
#define CP_SLOT_BYTES 28   // two 8-byte ping-pong tables, leader, next slot, edge id

typedef unsigned long long cp_u64;

struct CpTask {
    const double* P;  // ny x nx, row-major
    const double* x;
    const double* y;
    double level;
    int64_t woff;             // the task's slice of the bitmap and prefix words starts here
    int ny, nx, grid, first;  // first: the task that checks its grid for non-finite values
};

struct CpLat {
    const double* P;
    const double* x;
    const double* y;
    double L;
    int ny, nx, NH, E;  // NH horizontal edges, E edges in all
};

__device__ __forceinline__ CpLat cp_lattice(const CpTask& t) {
    CpLat g;
    g.P = t.P, g.x = t.x, g.y = t.y, g.L = t.level, g.ny = t.ny, g.nx = t.nx;
    g.NH = (t.ny + 2) * (t.nx + 1);
    g.E = g.NH + (t.ny + 1) * (t.nx + 2);
    return g;
}

// node (j, i) of the padded lattice: the ring is always below
__device__ __forceinline__ bool cp_real(const CpLat& g, int j, int i) { return j >= 1 && j <= g.ny && i >= 1 && i <= g.nx; }
__device__ __forceinline__ double cp_z(const CpLat& g, int j, int i) { return g.P[(j - 1) * g.nx + (i - 1)]; }
__device__ __forceinline__ bool cp_above(const CpLat& g, int j, int i) { return cp_real(g, j, i) && cp_z(g, j, i) > g.L; }

// edge id -> its lower-index node (j, i); returns whether the edge is horizontal
__device__ __forceinline__ bool cp_decode(const CpLat& g, int id, int* j, int* i) {
    if (id < g.NH) {
        *j = id / (g.nx + 1);
        *i = id - *j * (g.nx + 1);
        return true;
    }
    const int r = id - g.NH;
    *j = r / (g.nx + 2);
    *i = r - *j * (g.nx + 2);
    return false;
}

__device__ __forceinline__ bool cp_crossed(const CpLat& g, int id) {
    if (id >= g.E) return false;
    int j, i;
    const bool horiz = cp_decode(g, id, &j, &i);
    return cp_above(g, j, i) != (horiz ? cp_above(g, j, i + 1) : cp_above(g, j + 1, i));
}

// the edge on which the segment that starts on the crossed edge `id` ends
__device__ __forceinline__ int cp_next_edge(const CpLat& g, int id) {
    int j, i, k;  // (j, i) becomes the start cell, k the index of this edge on the cell's walk
    if (cp_decode(g, id, &j, &i)) {
        if (cp_above(g, j, i)) {
            k = 0;
        } else {
            k = 2;
            j -= 1;
        }
    } else {
        if (cp_above(g, j, i)) {
            k = 1;
            i -= 1;
        } else {
            k = 3;
        }
    }
    const int cj[4] = {j, j, j + 1, j + 1}, ci[4] = {i, i + 1, i + 1, i};
    bool a[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = cp_above(g, cj[c], ci[c]);
    int e = (k + 1) & 3;
    if (a[0] == a[2] && a[1] == a[3] && a[0] != a[1]) {  // saddle: the centre decides, below when the cell touches the ring
        bool centre = false;
        if (j >= 1 && j + 1 <= g.ny && i >= 1 && i + 1 <= g.nx)
            centre = 0.25 * (cp_z(g, j, i) + cp_z(g, j, i + 1) + cp_z(g, j + 1, i + 1) + cp_z(g, j + 1, i)) > g.L;
        e = centre ? ((k + 1) & 3) : ((k + 3) & 3);
    } else {
#pragma unroll
        for (int m = 3; m >= 1; --m) {
            const int kk = (k + m) & 3;
            if (!a[kk] && a[(kk + 1) & 3]) e = kk;
        }
    }
    // edge e of cell (j, i): bottom, right, top, left
    if (e == 0) return j * (g.nx + 1) + i;
    if (e == 1) return g.NH + j * (g.nx + 2) + i + 1;
    if (e == 2) return (j + 1) * (g.nx + 1) + i;
    return g.NH + j * (g.nx + 2) + i;
}

// the vertex on the crossed edge `id`: linear interpolation on an interior edge, the real node's own position (flag 1)
// on an edge to the ring
__device__ __forceinline__ void cp_vertex(const CpLat& g, int id, double* vx, double* vy, unsigned char* flag) {
    int j, i;
    if (cp_decode(g, id, &j, &i)) {  // (j, i)-(j, i+1), j in 1..ny
        *vy = g.y[j - 1];
        if (i == 0 || i == g.nx) {
            *vx = g.x[i == 0 ? 0 : g.nx - 1];
            *flag = 1;
        } else {
            const double za = cp_z(g, j, i), zb = cp_z(g, j, i + 1);
            const double f = (g.L - za) / (zb - za);
            *vx = g.x[i - 1] * (1.0 - f) + g.x[i] * f;
            *flag = 0;
        }
    } else {  // (j, i)-(j+1, i), i in 1..nx
        *vx = g.x[i - 1];
        if (j == 0 || j == g.ny) {
            *vy = g.y[j == 0 ? 0 : g.ny - 1];
            *flag = 1;
        } else {
            const double za = cp_z(g, j, i), zb = cp_z(g, j + 1, i);
            const double f = (g.L - za) / (zb - za);
            *vy = g.y[j - 1] * (1.0 - f) + g.y[j] * f;
            *flag = 0;
        }
    }
}

// exclusive prefix of v over the threads of the block, *total = the block's sum; sh holds CP_WAVES values
template <class T>
__device__ __forceinline__ T cp_block_exscan(T v, T* sh, T* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += u;
    }
    __syncthreads();  // the previous call's readers are done with sh
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < CP_WAVES; ++k) {
        const T c = sh[k];
        if (k < wv) base += c;
        tot += c;
    }
    *total = tot;
    return base + inc - v;
}

// cnt[t] = crossed edges of task t; big[t] = that number rounded up to even when the task's tables go to global scratch
// Also bits[w] = the crossed edges among the ids 64 w .. 64 w + 63 (one edge per lane, so neighbouring lanes read
// neighbouring grid values; CP_UNROLL words per step keep that many loads in flight) and pre[w] = their number.
#define CP_UNROLL 4
__global__ void __launch_bounds__(CP_THREADS) k_cp_count(const CpTask* __restrict__ tasks, const int* __restrict__ order,
                                                         long long* __restrict__ cnt, long long* __restrict__ big,
                                                         int* __restrict__ status, cp_u64* __restrict__ bits_all,
                                                         int* __restrict__ pre_all) {
    __shared__ int red[CP_WAVES];
    const int t = order[blockIdx.x];
    const CpTask tk = tasks[t];
    const CpLat g = cp_lattice(tk);
    cp_u64* bits = bits_all + tk.woff;
    int* pre = pre_all + tk.woff;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = (g.E + 63) >> 6;
    int c = 0;
    for (int w0 = wv * CP_UNROLL; w0 < W; w0 += CP_WAVES * CP_UNROLL) {
        bool crossed[CP_UNROLL];
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u) crossed[u] = cp_crossed(g, (w0 + u) * 64 + lane);
#pragma unroll
        for (int u = 0; u < CP_UNROLL; ++u) {
            const cp_u64 m = __ballot(crossed[u]);
            const int k = __popcll(m);
            c += k;
            if (lane == 0 && w0 + u < W) {
                bits[w0 + u] = m;
                pre[w0 + u] = k;
            }
        }
    }
    const int n = block_sum(lane == 0 ? c : 0, red);  // c is the wave's count in every lane
    int bad = 0;
    if (tk.first) {
        const int cells = g.ny * g.nx;
        for (int e = threadIdx.x; e < cells; e += CP_THREADS) bad |= !isfinite(g.P[e]);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        cnt[t] = n;
        big[t] = n > CP_LDS_SLOTS ? (n + 1) & ~1 : 0;
        if (tk.first) status[tk.grid] = bad ? 1 : 0;
    }
}

struct CpTables {
    cp_u64 *a, *b;       // ping-pong: (value << 32) | pointer
    int *leader, *next;  // next: the slot the segment ends on; later the loop base of a leader
    int* eid;
};

// Orders the n compacted crossed edges of one task and writes its vertices and loop starts.  Called with LDS tables or
// with global ones: inlined at both sites, so each copy addresses one kind of memory.
__device__ __forceinline__ void cp_order(const CpLat& g, const CpTables& tb, int n, const cp_u64* __restrict__ bits,
                                         const int* __restrict__ pre, int W, cp_u64* sh, double2* __restrict__ xy,
                                         unsigned char* __restrict__ flag, int* __restrict__ loop_start,
                                         long long* __restrict__ nloops) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const cp_u64 lo32 = 0xffffffffull;
    // compaction in id order, with the slot of the edge each segment ends on
    for (int w = wv; w < W; w += CP_WAVES) {
        const cp_u64 m = bits[w];
        if ((m >> lane) & 1ull) {
            const int s = pre[w] + __popcll(m & ((1ull << lane) - 1ull));
            const int id = w * 64 + lane;
            const int e2 = cp_next_edge(g, id);
            int s2 = pre[e2 >> 6] + __popcll(bits[e2 >> 6] & ((1ull << (e2 & 63)) - 1ull));
            if (s < n) {
                if (s2 >= n) s2 = s;
                tb.eid[s] = id;
                tb.next[s] = s2;
                tb.a[s] = ((cp_u64)s << 32) | (cp_u64)s2;
            }
        }
    }
    int rounds = 0;
    while ((1ll << rounds) < n) ++rounds;
    // leaders: after r rounds the value is the smallest slot among the 2^r slots from s on
    cp_u64 *src = tb.a, *dst = tb.b;
    for (int r = 0; r < rounds; ++r) {
        __syncthreads();
        for (int s = tid; s < n; s += CP_THREADS) {
            const cp_u64 u = src[s], v = src[(int)(u & lo32)];
            const cp_u64 mu = u >> 32, mv = v >> 32;
            dst[s] = ((mu < mv ? mu : mv) << 32) | (v & lo32);
        }
        cp_u64* t = src;
        src = dst, dst = t;
    }
    __syncthreads();
    // cut every cycle in front of its leader: (distance to the tail, pointer), the tail points at itself
    for (int s = tid; s < n; s += CP_THREADS) {
        const int ld = (int)(src[s] >> 32), nx = tb.next[s];
        tb.leader[s] = ld;
        dst[s] = nx == ld ? (cp_u64)s : ((1ull << 32) | (cp_u64)nx);
    }
    {
        cp_u64* t = src;
        src = dst, dst = t;
    }
    for (int r = 0; r < rounds; ++r) {
        __syncthreads();
        for (int s = tid; s < n; s += CP_THREADS) {
            const cp_u64 u = src[s], v = src[(int)(u & lo32)];
            dst[s] = (((u >> 32) + (v >> 32)) << 32) | (v & lo32);
        }
        cp_u64* t = src;
        src = dst, dst = t;
    }
    __syncthreads();
    // loops in leader order: (loops before, vertices before) by one scan of (1, length) over the leaders
    cp_u64 carry = 0;
    for (int c0 = 0; c0 < n; c0 += CP_THREADS) {
        const int s = c0 + tid;
        const bool lead = s < n && tb.leader[s] == s;
        const cp_u64 v = lead ? ((1ull << 32) | ((src[s] >> 32) + 1ull)) : 0ull;
        cp_u64 tot;
        const cp_u64 at = carry + cp_block_exscan<cp_u64>(v, sh, &tot);
        if (lead) {
            tb.next[s] = (int)(at & lo32);
            loop_start[(int)(at >> 32)] = (int)(at & lo32);
        }
        carry += tot;
    }
    if (tid == 0) *nloops = (long long)(carry >> 32);
    __syncthreads();
    for (int s = tid; s < n; s += CP_THREADS) {
        const int ld = tb.leader[s];
        const int pos = tb.next[ld] + (int)(src[ld] >> 32) - (int)(src[s] >> 32);
        double vx, vy;
        unsigned char fl;
        cp_vertex(g, tb.eid[s], &vx, &vy, &fl);
        if ((unsigned)pos < (unsigned)n) {
            xy[pos] = make_double2(vx, vy);
            flag[pos] = fl;
        }
    }
}

// Workgroup b takes task order[b].  voff / toff: the scanned counts of k_cp_count, whose bitmap and per-word counts it reads.
__global__ void __launch_bounds__(CP_THREADS) k_cp_paths(const CpTask* __restrict__ tasks, const int* __restrict__ order,
                                                         const long long* __restrict__ voff, const long long* __restrict__ toff,
                                                         const cp_u64* __restrict__ bits_all, int* __restrict__ pre_all,
                                                         char* __restrict__ tables, double2* __restrict__ xy,
                                                         unsigned char* __restrict__ flag, int* __restrict__ loop_start,
                                                         long long* __restrict__ nloops) {
    __shared__ __attribute__((aligned(16))) char lds[CP_LDS_SLOTS * CP_SLOT_BYTES];
    __shared__ cp_u64 sh[CP_WAVES];
    __shared__ int shi[CP_WAVES];
    const int tid = threadIdx.x, t = order[blockIdx.x];
    const long long v0 = voff[t];
    const int n = (int)(voff[t + 1] - v0);
    if (n == 0) {  // (the same for every thread)
        if (tid == 0) nloops[t] = 0;
        return;
    }
    const CpTask tk = tasks[t];
    const CpLat g = cp_lattice(tk);
    const cp_u64* bits = bits_all + tk.woff;
    int* pre = pre_all + tk.woff;
    const int W = (g.E + 63) >> 6;
    int carry = 0;  // the per-word counts become their exclusive prefix
    for (int c0 = 0; c0 < W; c0 += CP_THREADS) {
        const int i = c0 + tid;
        const int v = i < W ? pre[i] : 0;
        int tot;
        const int ex = cp_block_exscan<int>(v, shi, &tot);
        if (i < W) pre[i] = carry + ex;
        carry += tot;
    }
    __syncthreads();
    CpTables tb;
    if (n <= CP_LDS_SLOTS) {
        tb.a = (cp_u64*)lds;
        tb.b = tb.a + CP_LDS_SLOTS;
        tb.leader = (int*)(tb.b + CP_LDS_SLOTS);
        tb.next = tb.leader + CP_LDS_SLOTS;
        tb.eid = tb.next + CP_LDS_SLOTS;
        cp_order(g, tb, n, bits, pre, W, sh, xy + v0, flag + v0, loop_start + v0, nloops + t);
    } else {
        const int64_t cap = (n + 1) & ~1;
        tb.a = (cp_u64*)(tables + toff[t] * CP_SLOT_BYTES);
        tb.b = tb.a + cap;
        tb.leader = (int*)(tb.b + cap);
        tb.next = tb.leader + cap;
        tb.eid = tb.next + cap;
        cp_order(g, tb, n, bits, pre, W, sh, xy + v0, flag + v0, loop_start + v0, nloops + t);
    }
}

// the loop starts of every task, packed: loff = the scanned loop counts
__global__ void __launch_bounds__(256) k_cp_pack_loops(const long long* __restrict__ voff, const long long* __restrict__ loff,
                                                       const int* __restrict__ loop_start, int* __restrict__ loops) {
    const long long l0 = loff[blockIdx.x], nl = loff[blockIdx.x + 1] - l0;
    const int* src = loop_start + voff[blockIdx.x];
    for (long long l = threadIdx.x; l < nl; l += blockDim.x) loops[l0 + l] = src[l];
}

static int64_t cp_words(int ny, int nx) { return ((int64_t)(ny + 2) * (nx + 1) + (int64_t)(ny + 1) * (nx + 2) + 63) / 64; }

extern "C" {

int gd_contour_paths(gd_ctx* ctx, int32_t B, const void* d_grids, const int64_t* grid_off, const int32_t* ny, const int32_t* nx,
                     const double* x_axes, const int64_t* x_off, int64_t x_count, const double* y_axes, const int64_t* y_off,
                     int64_t y_count, const double* levels, int32_t nc, gd_paths_alloc_fn alloc, void* user,
                     int64_t* task_vert_off, int64_t* task_loop_off, int32_t* status_out) {
    GD_REQUIRE(ctx && d_grids && grid_off && ny && nx && x_axes && x_off && y_axes && y_off && levels && alloc && task_vert_off &&
                   task_loop_off && status_out && B > 0 && x_count > 0 && y_count > 0,
               "bad argument");
    GD_REQUIRE(nc >= 1 && nc <= CP_MAXC, "1..8 levels per grid");
    GD_REQUIRE((int64_t)B * nc < (1 << 30), "too many (grid, level) tasks for one call");
    int64_t words = 0;  // 64-edge bitmap words of all tasks
    for (int b = 0; b < B; ++b) {
        GD_REQUIRE(ny[b] >= 2 && ny[b] <= CP_MAX_SIDE && nx[b] >= 2 && nx[b] <= CP_MAX_SIDE, "grid side outside 2..4096");
        GD_REQUIRE(grid_off[b] >= 0, "negative grid offset");
        GD_REQUIRE(x_off[b] >= 0 && x_off[b] + nx[b] <= x_count && y_off[b] >= 0 && y_off[b] + ny[b] <= y_count,
                   "axis offset outside the axis arrays");
        words += (int64_t)nc * cp_words(ny[b], nx[b]);
    }
    const int T = B * nc;
    for (int t = 0; t < T; ++t) GD_REQUIRE(std::isfinite(levels[t]), "non-finite contour level");
    std::vector<int> order(T);  // largest task first (ties in task order): the few large grids do not become a tail
    for (int t = 0; t < T; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return cp_words(ny[a / nc], nx[a / nc]) > cp_words(ny[b / nc], nx[b / nc]); });

    ScratchPlan sp;
    auto d_tasks = sp.take<CpTask>(T);
    auto d_order = sp.take<int>(T);
    auto d_x = sp.take<double>(x_count);
    auto d_y = sp.take<double>(y_count);
    const int64_t meta_bytes = sp.bytes();
    auto d_cnt = sp.take<long long>(T + 1), d_big = sp.take<long long>(T + 1), d_nl = sp.take<long long>(T + 1);
    auto d_st = sp.take<int>(B);
    auto d_bits = sp.take<cp_u64>(words);
    auto d_pre = sp.take<int>(words);
    GD_TRY(sp.get(ctx));

    std::vector<char> meta((size_t)meta_bytes, 0);
    CpTask* tasks = (CpTask*)(meta.data() + d_tasks.off);
    memcpy(meta.data() + d_order.off, order.data(), (size_t)T * 4);
    memcpy(meta.data() + d_x.off, x_axes, (size_t)x_count * 8);
    memcpy(meta.data() + d_y.off, y_axes, (size_t)y_count * 8);
    int64_t woff = 0;
    for (int b = 0; b < B; ++b) {
        for (int c = 0; c < nc; ++c) {
            CpTask& tk = tasks[b * nc + c];
            tk.P = (const double*)d_grids + grid_off[b];
            tk.x = d_x + x_off[b];
            tk.y = d_y + y_off[b];
            tk.level = levels[b * nc + c];
            tk.woff = woff;
            woff += cp_words(ny[b], nx[b]);
            tk.ny = ny[b], tk.nx = nx[b], tk.grid = b, tk.first = c == 0;
        }
    }
    GD_TRY(gd_h2d(ctx, d_tasks, meta.data(), (size_t)meta_bytes));
    k_cp_count<<<T, CP_THREADS, 0, ctx->stream>>>(d_tasks, d_order, d_cnt, d_big, d_st, d_bits, d_pre);
    GD_KERNEL_CHECK();
    long long V = 0, Vbig = 0, L = 0;
    GD_TRY(gd_tile_offsets(ctx, d_cnt, T, &V));
    GD_TRY(gd_tile_offsets(ctx, d_big, T, &Vbig));
    GD_TRY(gd_fetch(ctx, status_out, d_st, (size_t)B * 4));
    GD_TRY(gd_stream_sync(ctx));  // the meta block was pageable: the copy has read it by now
    for (int t = 0; t <= T; ++t) task_vert_off[t] = task_loop_off[t] = 0;
    for (int b = 0; b < B; ++b)
        if (status_out[b]) return GD_OK;  // a non-finite grid: the caller reports it, nothing is traced
    if (V == 0) return GD_OK;

    ScratchPlan work;
    auto d_tab = work.take<char>(Vbig * CP_SLOT_BYTES);
    auto d_xy = work.take<double2>(V);
    auto d_ls = work.take<int>(V);
    auto d_loops = work.take<int>(V);
    auto d_flag = work.take<unsigned char>(V);
    GD_TRY(work.get2(ctx));
    k_cp_paths<<<T, CP_THREADS, 0, ctx->stream>>>(d_tasks, d_order, d_cnt, d_big, d_bits, d_pre, d_tab, d_xy, d_flag, d_ls, d_nl);
    GD_KERNEL_CHECK();
    GD_TRY(gd_tile_offsets(ctx, d_nl, T, &L));
    k_cp_pack_loops<<<T, 256, 0, ctx->stream>>>(d_cnt, d_nl, d_ls, d_loops);
    GD_KERNEL_CHECK();
    GD_TRY(gd_fetch(ctx, task_vert_off, d_cnt, (size_t)(T + 1) * 8));
    GD_TRY(gd_fetch(ctx, task_loop_off, d_nl, (size_t)(T + 1) * 8));
    GD_TRY(gd_stream_sync(ctx));
    void* h_xy = alloc(user, GD_PATHS_XY, V);
    void* h_flag = alloc(user, GD_PATHS_FLAG, V);
    void* h_loops = alloc(user, GD_PATHS_LOOPS, L);
    if (!h_xy || !h_flag || !h_loops) return gd_fail(ctx, GD_ERR_NOMEM, "the caller could not allocate the result arrays");
    GD_TRY(gd_fetch(ctx, h_xy, d_xy, (size_t)V * 16));
    GD_TRY(gd_fetch(ctx, h_flag, d_flag, (size_t)V));
    GD_TRY(gd_fetch(ctx, h_loops, d_loops, (size_t)L * 4));
    GD_TRY(gd_stream_sync(ctx));
    return GD_OK;
}

}  // extern "C"
