// gd_density2d_batch: the native entry for a batch of parameter pairs.  The plan and the choreography live in
// batch2d.hpp (host C++, shared with the CPU test harness); this file binds its table of device entry points to the
// library's own C ABI and keeps the per-context state (block pool, cached index columns, the last call in flight).
#include "batch1d.hpp"
#include "batch2d.hpp"
#include "ctx.hpp"

namespace {

gd_ctx* C(void* h) { return (gd_ctx*)h; }

// ---- work enqueued ahead by gd_prepare_params --------------------------------------------------------------------------
// A piece is one enqueue-and-record: what it was launched with, the event behind its last kernel, where its result lands.
// It is used at most once, by the binding whose arguments are the same to the bit; whoever finds it first otherwise waits
// for its event (finite kernels) and discards it.  No piece outlives the sample set it read (drop_ahead).
struct Ahead {
    // the bindings run on the batched call's N_eff and binning threads, and each waits for its piece's event under its
    // piece's lock: one lock per piece, so that the binning thread never waits for the lag sums
    std::mutex mu_neff, mu_prebin;
    struct {
        bool pending = false;
        std::vector<int32_t> cols;
        std::vector<double> inv4s2;
        std::vector<int64_t> lags;
        int64_t N = 0;
        const double *samples = nullptr, *weights = nullptr;
        gd_kde_lag_ticket t{};
    } neff;
    struct {
        bool pending = false;
        std::vector<int32_t> cols;
        std::vector<void*> bufs;
    } prebin;
    hipEvent_t ev_neff = nullptr, ev_prebin = nullptr;
    void* d_block = nullptr;  // the lag sums' tables and partials
    int64_t d_bytes = 0;
    double* pinned = nullptr;  // ... and the partials on the host
    int64_t pinned_bytes = 0;
    unsigned long long* bad_pinned = nullptr;  // out-of-range counts of the index columns (2 words per column)
    int64_t bad_words = 0;
    std::atomic<int64_t> enqueued{0}, consumed{0}, discarded{0};
};

// every index column a pending piece is writing -> the context that owns the piece.  Whoever is about to read or rewrite such
// a column -- on whatever context's stream -- finds the piece through the column itself (meet_prebin_ahead).
std::mutex g_prebin_mu;
std::map<const void*, gd_ctx*> g_prebin_owner;

Ahead* ahead_if(gd_ctx* ctx) {
    return ctx && ctx->batch_state ? (Ahead*)((gdb::State*)ctx->batch_state)->ahead : nullptr;
}

// waits for a pending piece's event and forgets the piece (the piece's lock held); `used`: it was consumed, not discarded
void settle_neff(gd_ctx* ctx, Ahead& A, bool used) {
    if (!A.neff.pending) return;
    (void)hipEventSynchronize(A.ev_neff);
    A.neff.pending = false;
    ((gdb::State*)ctx->batch_state)->neff_ahead.store(false);
    ++(used ? A.consumed : A.discarded);
}
// The index-column piece: its event is waited for, and every column of it that has a sample outside the grid (or whose
// kernels did not run) is marked stale in the owner's cache -- except those in `rebinned`, which the caller is binning again --
// whether the piece is then used or dropped: a column stays valid only behind a completed event and a zero count.
// Returns the columns found bad.
std::vector<const void*> settle_prebin(gd_ctx* owner, Ahead& A, bool used, const std::vector<const void*>& rebinned = {}) {
    std::vector<const void*> bad;
    if (!A.prebin.pending) return bad;
    const bool ran = hipEventSynchronize(A.ev_prebin) == hipSuccess;
    gdb::State& st = *(gdb::State*)owner->batch_state;
    const int m = (int)A.prebin.cols.size();
    for (int c = 0; c < m; ++c) {
        const void* buf = A.prebin.bufs[c];
        if (ran && A.bad_pinned[A.bad_pinned[m + c]] == 0) continue;
        bad.push_back(buf);
        if (std::find(rebinned.begin(), rebinned.end(), buf) != rebinned.end()) continue;
        gdb::IndexCache{st}.mark_stale((int)A.prebin.cols[c], 256, gdb::IndexCache::kBytes, buf);
    }
    A.prebin.pending = false;
    {
        std::lock_guard<std::mutex> g(g_prebin_mu);
        for (const void* buf : A.prebin.bufs) g_prebin_owner.erase(buf);
    }
    ++((used && bad.empty()) ? A.consumed : A.discarded);
    return bad;
}
// every pending piece of the context: waited for and discarded (a new preparation, the end of a batched call that did not
// ask for it, a change of the sample set, teardown)
void drop_ahead(gd_ctx* ctx) {
    Ahead* A = ahead_if(ctx);
    if (!A) return;
    {
        std::lock_guard<std::mutex> g(A->mu_neff);
        settle_neff(ctx, *A, false);
    }
    std::lock_guard<std::mutex> g(A->mu_prebin);
    (void)settle_prebin(ctx, *A, false);
}

// the lag sums of a pending piece, if these are its arguments; else the piece is gone when this returns
bool take_neff_ahead(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* inv4s2, const int64_t* lags, int32_t nlags,
                     double* out) {
    Ahead* A = ahead_if(ctx);
    if (!A) return false;
    std::lock_guard<std::mutex> g(A->mu_neff);
    if (!A->neff.pending) return false;
    const auto& p = A->neff;
    // the same launch: N, the lag list, and the same columns with the same kernel widths -- in any order (a column's partial
    // sums depend on its own data, its width, the lags and the number of blocks, which follows from the column COUNT)
    bool same = p.N == ctx->N && p.samples == ctx->cols && p.weights == ctx->w && ctx->w_sel == 0 && cols && inv4s2 && lags &&
                (int32_t)p.cols.size() == ncols && (int32_t)p.lags.size() == nlags &&
                memcmp(p.lags.data(), lags, (size_t)nlags * 8) == 0;
    std::vector<int> row_of(same ? ncols : 0, -1);
    for (int c = 0; c < ncols && same; ++c) {
        for (int q = 0; q < ncols && row_of[c] < 0; ++q)
            if (p.cols[q] == cols[c] && memcmp(&p.inv4s2[q], &inv4s2[c], 8) == 0) row_of[c] = q;
        same = row_of[c] >= 0;
        for (int b = 0; b < c && same; ++b) same = cols[b] != cols[c];  // (a column listed twice: today's path)
    }
    const bool ran = hipEventSynchronize(A->ev_neff) == hipSuccess;
    settle_neff(ctx, *A, same && ran);
    if (!(same && ran)) return false;
    std::vector<double> sums((size_t)ncols * nlags);
    gd_kde_lag_sums_reduce(&p.t, A->pinned, sums.data());
    for (int c = 0; c < ncols; ++c) memcpy(out + (size_t)c * nlags, &sums[(size_t)row_of[c] * nlags], (size_t)nlags * 8);
    return true;
}

// A launch that is about to read the byte-index columns ix / iy (B each, may be null) or to write d_idx (ncols), on any
// context's stream, meets the pending piece that is writing one of them: the piece is found through the columns, its event is
// waited for on the host and its counts of samples outside the grid are read, as the fused launch would have read them.  The
// piece was consumed when a column of it is read without being binned again.  GD_ERR_SOLVER: such a column has a sample
// outside the grid (it is marked stale; the caller takes the u16 path, as after the fused launch's own count).
int meet_prebin_ahead(gd_ctx* on, int32_t ncols, void* const* d_idx, int32_t B, const void* const* ix, const void* const* iy) {
    gd_ctx* owner = nullptr;
    {
        std::lock_guard<std::mutex> g(g_prebin_mu);
        if (g_prebin_owner.empty()) return 0;
        auto look = [&](const void* p) {
            if (owner) return;
            auto it = g_prebin_owner.find(p);
            if (it != g_prebin_owner.end()) owner = it->second;
        };
        for (int q = 0; q < ncols && !owner; ++q) look(d_idx[q]);
        for (int q = 0; q < B && !owner; ++q) {
            if (ix) look(ix[q]);
            if (iy) look(iy[q]);
        }
    }
    Ahead* A = owner && gd_ctx_alive(owner) ? ahead_if(owner) : nullptr;
    if (!A) return 0;
    std::lock_guard<std::mutex> g(A->mu_prebin);
    if (!A->prebin.pending) return 0;
    std::vector<const void*> rebinned, fresh;  // the piece's columns this launch bins again / reads as the piece left them
    for (const void* buf : A->prebin.bufs) {
        bool again = false, read = false;
        for (int q = 0; q < ncols && !again; ++q) again = d_idx[q] == buf;
        for (int q = 0; q < B && !read; ++q) read = (ix && ix[q] == buf) || (iy && iy[q] == buf);
        if (again)
            rebinned.push_back(buf);
        else if (read)
            fresh.push_back(buf);
    }
    const std::vector<const void*> bad = settle_prebin(owner, *A, !fresh.empty(), rebinned);
    for (const void* buf : fresh)
        if (std::find(bad.begin(), bad.end(), buf) != bad.end())
            return gd_fail(on, GD_ERR_SOLVER, "samples outside the byte-index grid: use the u16 path");
    return 0;
}

const gdb::Ops kOps = {
    /* bind_thread */ [](void* h) { return gd_bind_thread(C(h)); },
    /* num_rows */ [](void* h, int64_t* N, int64_t* n) { return gd_num_rows(C(h), N, n); },
    /* weights_kind */
    [](void* h, int32_t* hw) {  // 0: unit weights, 1: weights, 2: real (non-integral) weights with a known total
        gd_ctx* c = C(h);
        *hw = c->w == nullptr ? 0 : ((!c->w8 && !c->w_integral && c->w_sum > 1e-200 && c->w_sum < 1e200) ? 2 : 1);
        return 0;
    },
    /* dev_alloc */ [](void* h, int64_t bytes, void** out) { return gd_dev_alloc(C(h), bytes, out); },
    /* dev_free */ [](void* h, void* p) { return gd_dev_free(C(h), p); },
    /* prebin8_batch */
    [](void* h, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, int32_t F, void* const* d_idx,
       int64_t* bad) {
        (void)meet_prebin_ahead(C(h), ncols, d_idx, 0, nullptr, nullptr);  // (the columns are written again either way)
        return gd_prebin8_batch(C(h), cols, ncols, binmin, width, F, d_idx, bad);
    },
    /* hist2d_prebinned8 */
    [](void* h, int32_t B, const void* const* ix, const void* const* iy, void* d_hist) {
        const int rc = meet_prebin_ahead(C(h), 0, nullptr, B, ix, iy);
        if (rc) return rc;
        return gd_hist2d_prebinned8(C(h), B, ix, iy, d_hist);
    },
    /* prebin8_hist2d */
    [](void* h, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, void* const* d_idx, int64_t* bad,
       int32_t B, const void* const* ix, const void* const* iy, void* d_hist) {
        const int rc = meet_prebin_ahead(C(h), ncols, d_idx, B, ix, iy);
        if (rc) return rc;
        return gd_prebin8_hist2d(C(h), cols, ncols, binmin, width, d_idx, bad, B, ix, iy, d_hist);
    },
    /* prebin */
    [](void* h, int32_t col, double binmin, double width, int32_t F, void* d_idx) {
        return gd_prebin(C(h), col, binmin, width, F, d_idx);
    },
    /* hist2d_prebinned */
    [](void* h, int32_t B, const void* const* ix, const void* const* iy, int32_t F, void* d_hist) {
        return gd_hist2d_prebinned(C(h), B, ix, iy, F, d_hist);
    },
    /* minmax_affine */
    [](void* h, int32_t B, const int32_t* ci, const int32_t* cj, const double* a, const double* b, double* out) {
        return gd_minmax_affine(C(h), B, ci, cj, a, b, out);
    },
    /* hist2d_sheared */
    [](void* h, int32_t B, const int32_t* ci, const int32_t* cj, const double* r0, const double* r1, const double* xmin,
       const double* dx, const double* ymin, const double* dy, int32_t F, void* d_hist) {
        return gd_hist2d_sheared(C(h), B, ci, cj, r0, r1, xmin, dx, ymin, dy, F, d_hist);
    },
    /* kopt2d */
    [](void* h, int32_t B, int32_t F, const void* d_hist, const double* neff, const int32_t* do_corr, const double* fallback_t,
       const double* corr, double* out) { return gd_kopt2d(C(h), B, F, d_hist, neff, do_corr, fallback_t, corr, out); },
    /* gather_items */
    [](void* h, void* d_dst, int64_t dst_first, const void* d_src, const int32_t* index, int32_t count, int64_t item_bytes) {
        return gd_gather_items(C(h), (char*)d_dst + dst_first * item_bytes, d_src, index, count, item_bytes);
    },
    /* density2d_enqueue */
    [](void* h, int32_t B, int32_t F, const void* d_hist, const int32_t* hist_index, const double* rx, const double* ry,
       const double* corr, const int32_t* winw, const int32_t* flags, int32_t bco, int32_t mbc, void* d_P, int32_t* status_pinned) {
        return gd_density2d_enqueue_indexed(C(h), B, F, d_hist, hist_index, rx, ry, corr, winw, flags, bco, mbc, d_P, status_pinned);
    },
    /* d2h_async */ [](void* h, void* dst, const void* d_src, int64_t bytes) { return gd_memcpy_d2h_async(C(h), dst, d_src, bytes); },
    /* copy_mark */ [](void* h, int32_t* token) { return gd_copy_mark(C(h), token); },
    /* copy_wait: a context destroyed meanwhile has synchronised its copy stream on the way out */
    [](void* h, int32_t token) {
        if (!gd_ctx_alive(C(h))) return 0;
        const int rc = gd_copy_wait(C(h), token);
        return rc == GD_ERR_BADARG ? 0 : rc;  // (a new context at the old address: no such mark)
    },
    /* copy_sync */ [](void* h) { return gd_ctx_alive(C(h)) ? gd_copy_sync(C(h)) : 0; },
    /* contour_levels */
    [](void* h, int32_t B, int32_t F, const void* d_P, const double* contours, int32_t nc, double* out, int32_t* status) {
        return gd_contour_levels(C(h), B, F, d_P, contours, nc, out, status);
    },
    /* autocov_lags_batch */
    [](void* h, const int32_t* cols, int32_t ncols, const double* means, int64_t k0, int32_t nlags, double* out) {
        return gd_autocov_lags_batch(C(h), cols, ncols, means, k0, nlags, out);
    },
    /* kde_lag_sums_batch */
    [](void* h, const int32_t* cols, int32_t ncols, const double* inv4s2, const int64_t* lags, int32_t nlags, double* out) {
        if (take_neff_ahead(C(h), cols, ncols, inv4s2, lags, nlags, out)) return 0;
        return gd_kde_lag_sums_batch(C(h), cols, ncols, inv4s2, lags, nlags, out);
    },
    /* kde_lag_sums */
    [](void* h, int32_t col, double inv4s2, const int64_t* lags, int32_t nlags, double* out) {
        return gd_kde_lag_sums(C(h), col, inv4s2, lags, nlags, out);
    },
    /* last_error */ [](void* h) { return gd_last_error(C(h)); },
    /* create_aux */
    [](void* h, void** aux) {
        gd_ctx* a = nullptr;
        int rc = gd_create(C(h)->device, &a);
        if (rc == 0) rc = gd_attach_samples(a, C(h));
        if (rc == 0) rc = gd_stream_priority(a, 1);  // small latency-critical kernels (get_h) beside saturating launches
        if (rc) {
            if (a) gd_destroy(a);
            return gd_fail(C(h), rc, "could not create the third context of a batched call");
        }
        *aux = a;
        return 0;
    },
    /* destroy_aux */
    [](void* aux) {
        gd_destroy(C(aux));
        return 0;
    },
    /* kopt2d_enqueue */
    [](void* h, int32_t B, int32_t F, const void* d_hist, const double* neff, const int32_t* do_corr, const double* fallback_t,
       const double* corr, void* d_rows, int32_t* ticket) {
        return gd_kopt2d_enqueue(C(h), B, F, d_hist, neff, do_corr, fallback_t, corr, d_rows, ticket);
    },
    /* kopt2d_finish */
    [](void* h, void* stage_a_h, int32_t ticket, int32_t B, void* d_rows, double* out) {
        return gd_kopt2d_finish(C(h), C(stage_a_h), ticket, B, d_rows, out);
    },
    /* comm_world */ [](void* h) { return C(h)->comm ? C(h)->comm_world : 0; },
    /* comm_allreduce_sum */ [](void* h, double* inout, int64_t count) { return gd_comm_allreduce_sum(C(h), inout, count); },
    /* stream_priority */ [](void* ctx, int level) { return gd_stream_priority(C(ctx), level); },
    /* prebin_batch */
    [](void* h, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, int32_t F, void* const* d_idx) {
        return gd_prebin_batch(C(h), cols, ncols, binmin, width, F, d_idx);
    },
};

const gdb::Ops1D kOps1D = {
    /* hist1d_dev */
    [](void* h, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, int32_t F, void* d_hist) {
        return gd_hist1d_dev(C(h), cols, ncols, binmin, width, F, d_hist);
    },
    /* isj1d_dev */
    [](void* h, int32_t B, int32_t F, const void* d_hist, const double* neff, double* hfrac, int32_t* status) {
        return gd_isj1d_dev(C(h), B, F, d_hist, neff, hfrac, status);
    },
    /* density1d_dev */
    [](void* h, int32_t B, int32_t F, const void* d_hist, const double* smooth, const int32_t* winw, const int32_t* flags,
       int32_t bco, int32_t mbc, double* P_out, int32_t* status) {
        return gd_density1d_dev(C(h), B, F, d_hist, smooth, winw, flags, bco, mbc, P_out, status);
    },
    /* fetch */
    [](void* h, void* dst, const void* d_src, int64_t bytes) {
        const int rc = gd_fetch(C(h), dst, d_src, (size_t)bytes);
        return rc ? rc : gd_stream_sync(C(h));
    },
};

void release_state(gd_ctx* ctx, bool destroy) {
    gdb::State* st = (gdb::State*)ctx->batch_state;
    if (!st) return;
    drop_ahead(ctx);  // (its kernels read the sample set and write index columns that are about to go)
    gdb::release_all(*st, kOps, ctx);
    if (destroy) {
        if (Ahead* A = (Ahead*)st->ahead) {
            if (A->ev_neff) (void)hipEventDestroy(A->ev_neff);
            if (A->ev_prebin) (void)hipEventDestroy(A->ev_prebin);
            if (A->d_block) (void)hipFree(A->d_block);
            if (A->pinned) (void)hipHostFree(A->pinned);
            if (A->bad_pinned) (void)hipHostFree(A->bad_pinned);
            delete A;
            st->ahead = nullptr;
        }
        delete st;
        ctx->batch_state = nullptr;
    }
}

gdb::State& state_of(gd_ctx* ctx) {
    if (!ctx->batch_state) {
        ctx->batch_state = new gdb::State();
        ctx->batch_state_release = release_state;
    }
    return *(gdb::State*)ctx->batch_state;
}

Ahead& ahead_of(gd_ctx* ctx) {
    gdb::State& st = state_of(ctx);
    if (!st.ahead) st.ahead = new Ahead();
    return *(Ahead*)st.ahead;
}

bool prepare_ahead_enabled() {
    const char* e = getenv("GDHIP_PREPARE_AHEAD");
    return !(e && atoi(e) == 0);
}

// The index columns of the base grid for `cols`, on twin's stream into the owner's index-column cache.  The cache entries
// carry the edges from now on: the batched call finds them valid, and the binding of its fused launch waits for the event.
int enqueue_prebin_ahead(gd_ctx* ctx, gd_ctx* twin, Ahead& A, const int32_t* cols, int32_t ncols, const double* minmax,
                         const gd_prepared_param* recs) {
    gdb::State& st = state_of(ctx);
    gdb::Pool pool{st, kOps, ctx};
    std::vector<int32_t> want;
    std::vector<double> b0, w;
    for (int c = 0; c < ncols; ++c) {
        gd_param2d p;
        memset(&p, 0, sizeof p);
        p.range_min = recs[c].range_min, p.range_max = recs[c].range_max, p.param_min = minmax[2 * c], p.param_max = minmax[2 * c + 1];
        p.has_limits_bot = recs[c].has_limits_bot, p.has_limits_top = recs[c].has_limits_top;
        double lo, hi;
        gdb::bin_edges(p, &lo, &hi);
        const double fw = (hi - lo) / 255;
        if (!(fw > 0) || !std::isfinite(fw) || !std::isfinite(lo)) continue;
        want.push_back(cols[c]), b0.push_back(lo), w.push_back(fw);
    }
    gdb::IndexCache cache{st};
    gdb::IndexCache::Stale stale;
    int rc = cache.stale(pool, want, 256, gdb::IndexCache::kBytes, ctx->N, b0.data(), w.data(), stale);
    if (rc) return rc;
    const int m = (int)stale.cols.size();
    if (!m) return 0;
    if (A.bad_words < 2 * (int64_t)m) {
        if (A.bad_pinned) (void)hipHostFree(A.bad_pinned);
        A.bad_pinned = nullptr, A.bad_words = 0;
        if (hipHostMalloc((void**)&A.bad_pinned, (size_t)(2 * m + 64) * 8, hipHostMallocDefault) != hipSuccess) return GD_ERR_NOMEM;
        A.bad_words = 2 * m + 64;
    }
    memset(A.bad_pinned, 0xff, (size_t)m * 8);  // (a count that never arrives reads as out of range)
    if (!A.ev_prebin && hipEventCreateWithFlags(&A.ev_prebin, hipEventDisableTiming) != hipSuccess) return GD_ERR_HIP;
    rc = gd_prebin8_enqueue(twin, stale.cols.data(), m, stale.binmin.data(), stale.width.data(), stale.bufs.data(), A.bad_pinned);
    // (whatever was enqueued before a failure still writes the columns: the event goes behind it either way)
    const bool recorded = hipEventRecord(A.ev_prebin, twin->stream) == hipSuccess;
    if (rc || !recorded) {
        (void)hipStreamSynchronize(twin->stream);
        return rc ? rc : GD_ERR_HIP;
    }
    cache.commit(stale, 256, gdb::IndexCache::kBytes);  // (the counts arrive with the event: settle_prebin)
    A.prebin.cols = stale.cols, A.prebin.bufs = stale.bufs, A.prebin.pending = true;
    {
        std::lock_guard<std::mutex> g(g_prebin_mu);
        for (void* buf : stale.bufs) g_prebin_owner[buf] = ctx;
    }
    ++A.enqueued;
    return 0;
}

// The first launch of the N_eff lag sums of `cols` on ctx's stream, planned by the batched call's own lag_plan
int enqueue_neff_ahead(gd_ctx* ctx, Ahead& A, const int32_t* cols, int32_t ncols, const double* probe, const double* vars,
                       const double* err, const gd_prepared_param* recs) {
    const int64_t N = ctx->N;
    if (std::min<int64_t>(8, N / 10 + 1) != 8) return 0;  // (the probe holds 8 lags)
    for (size_t q = 0; q < (size_t)ncols * 8; ++q)
        if (std::isnan(probe[q])) return 0;
    std::vector<double> sr(ncols);
    for (int c = 0; c < ncols; ++c) sr[c] = recs[c].sigma_range;
    gdb::LagPlan lp;
    if (gdb::lag_plan(N, ncols, 8, probe, vars, sr.data(), err, gdb::kNeffMinCorr, lp) >= 0) return 0;  // a chain that outlasts the probe
    const int L = (int)lp.lags.size();
    for (int64_t k : lp.lags)
        if (!(k > 0 && k < N)) return 0;
    const int64_t partials = gd_kde_lag_sums_partials(ctx, ncols, L);
    if (partials <= 0) return 0;
    const int64_t dev_bytes = partials * 8 + (int64_t)ncols * 16 + 4096, host_bytes = partials * 8;
    if (A.d_bytes < dev_bytes) {
        if (A.d_block) (void)hipFree(A.d_block);
        A.d_block = nullptr, A.d_bytes = 0;
        if (hipMalloc(&A.d_block, (size_t)dev_bytes) != hipSuccess) return GD_ERR_NOMEM;
        A.d_bytes = dev_bytes;
    }
    if (A.pinned_bytes < host_bytes) {
        if (A.pinned) (void)hipHostFree(A.pinned);
        A.pinned = nullptr, A.pinned_bytes = 0;
        if (hipHostMalloc((void**)&A.pinned, (size_t)host_bytes, hipHostMallocDefault) != hipSuccess) return GD_ERR_NOMEM;
        A.pinned_bytes = host_bytes;
    }
    if (!A.ev_neff && hipEventCreateWithFlags(&A.ev_neff, hipEventDisableTiming) != hipSuccess) return GD_ERR_HIP;
    const int rc = gd_kde_lag_sums_enqueue(ctx, cols, ncols, lp.inv4s2.data(), lp.lags.data(), L, A.d_block, A.pinned, &A.neff.t);
    const bool recorded = hipEventRecord(A.ev_neff, ctx->stream) == hipSuccess;
    if (rc || !recorded) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc ? rc : GD_ERR_HIP;
    }
    A.neff.cols.assign(cols, cols + ncols), A.neff.inv4s2 = lp.inv4s2, A.neff.lags = lp.lags;
    A.neff.N = N, A.neff.samples = ctx->cols, A.neff.weights = ctx->w, A.neff.pending = true;
    state_of(ctx).neff_ahead.store(true);
    ++A.enqueued;
    return 0;
}

}  // namespace

extern "C" {

int gd_prepare_params(gd_ctx* ctx, gd_ctx* twin, const gd_prepare_settings* settings, const int32_t* cols, int32_t ncols,
                      const double* targets, const double* minmax, const double* means, const double* vars, const double* err,
                      const double* limits, double* quantiles_out, double* probe_out, int32_t* probe_done,
                      gd_prepared_param* recs) {
    GD_REQUIRE(ctx && settings && cols && targets && minmax && means && vars && err && limits && quantiles_out && probe_out &&
                   probe_done && recs && ncols > 0,
               "bad argument");
    GD_REQUIRE(ctx->cols, "no samples uploaded");
    GD_REQUIRE_SAMPLE_COLUMNS(cols, ncols);
    GD_HIP(hipSetDevice(ctx->device));
    drop_ahead(ctx);  // (pieces of an earlier preparation nobody asked for)
    GD_TRY(gd_quantiles_mm_probe(ctx, cols, ncols, 0, ctx->N, targets, 11, minmax, quantiles_out, means, probe_out, probe_done));
    for (int c = 0; c < ncols; ++c)
        gdb::prepare_tail(quantiles_out + (size_t)11 * c, minmax[2 * c], minmax[2 * c + 1], err[c], limits[2 * c], limits[2 * c + 1], &recs[c]);
    if (!settings->ahead || !prepare_ahead_enabled() || ctx->w_sel != 0) return GD_OK;
    // From here on nothing may fail the call: a piece that cannot be enqueued is work the batched call does itself.
    try {
        Ahead& A = ahead_of(ctx);
        std::lock_guard<std::mutex> g1(A.mu_neff), g2(A.mu_prebin);
        // the binning chain's launches go out before the N_eff launch, whose resident blocks fill every wave slot.  Index
        // columns are enqueued ahead for unit weights only: with real weights (which the batched call also bins from byte
        // indices, partitioned by stripe in several launches of its own) the lag sums alone go out ahead
        int rc = 0;
        if ((settings->ahead & 2) && twin && twin != ctx && twin->cols == ctx->cols && !ctx->w && settings->fine_bins_2D == 256 &&
            (int64_t)ncols * (ncols - 1) / 2 >= gdb::kByteIndexMinPairs)
            rc = enqueue_prebin_ahead(ctx, twin, A, cols, ncols, minmax, recs);
        if (!rc && (settings->ahead & 1) && settings->auto_bandwidth && !settings->uncorrelated_sampler && *probe_done)
            rc = enqueue_neff_ahead(ctx, A, cols, ncols, probe_out, vars, err, recs);
        if (rc) (void)hipGetLastError();
    } catch (const std::exception&) {
    }
    return GD_OK;
}

int gd_prepare_ahead_counts(gd_ctx* ctx, int64_t* out3) {
    GD_REQUIRE(ctx && out3, "null argument");
    out3[0] = out3[1] = out3[2] = 0;
    if (Ahead* A = ahead_if(ctx)) out3[0] = A->enqueued.load(), out3[1] = A->consumed.load(), out3[2] = A->discarded.load();
    return GD_OK;
}

int gd_batch2d_grid_sizes(const gd_batch2d_settings* settings, int32_t n, const double* corr, const int32_t* pairs, int32_t P,
                          int32_t* F_out) {
    if (!settings || !corr || (!pairs && P > 0) || (!F_out && P > 0) || n <= 0 || P < 0) return GD_ERR_BADARG;
    for (int k = 0; k < 2 * P; ++k)
        if (pairs[k] < 0 || pairs[k] >= n) return GD_ERR_BADARG;
    gdb::PairScalars ps;
    gdb::pair_scalars(*settings, n, corr, pairs, P, ps);
    for (int k = 0; k < P; ++k) F_out[k] = ps.F[k];
    return GD_OK;
}

int gd_density2d_batch(gd_ctx* ctx, gd_ctx* twin, const gd_batch2d_settings* settings, gd_param2d* params, int32_t n,
                       const double* corr, const double* cov, const double* lag_probe, const int32_t* pairs, int32_t P,
                       gd_neff_exchange_fn exchange, void* exchange_user, void* grids_pinned, int64_t grids_doubles,
                       int32_t* status_pinned, double* meta, double* levels, int32_t* level_status, int32_t* tokens_out2) {
    GD_REQUIRE(ctx && settings && params && corr && cov && tokens_out2 && n > 0 && P >= 0, "bad argument");
    GD_REQUIRE(P == 0 || (pairs && grids_pinned && status_pinned && meta), "bad argument");
    GD_REQUIRE(ctx->cols, "no samples uploaded");
    GD_REQUIRE(!twin || (twin != ctx && twin->cols == ctx->cols), "the second context must be attached to the first (gd_attach_samples)");
    GD_REQUIRE(ctx->w_sel == 0, "auxiliary weights are selected");
    GD_REQUIRE(!settings->want_levels || (settings->contours && settings->ncontours > 0 && levels && level_status), "contour levels requested without room for them");
    GD_HIP(hipSetDevice(ctx->device));
    int rc;
    try {
        gdb::Call call(state_of(ctx), kOps, ctx, twin, *settings, params, n, corr, cov, lag_probe, pairs, P, exchange, exchange_user,
                       (double*)grids_pinned, grids_doubles, status_pinned, meta, levels, level_status);
        rc = call.run(tokens_out2);
        if (rc) ctx->err = call.err;
    } catch (const std::exception& e) {
        rc = gd_fail(ctx, GD_ERR_NOMEM, "gd_density2d_batch: %s", e.what());
    }
    drop_ahead(ctx);  // (a piece this call had no use for: other columns, another grid size, N_eff known already)
    return rc;
}

int gd_density1d_batch(gd_ctx* ctx, const gd_density1d_settings* settings, gd_param2d* params, int32_t n, const int32_t* cols,
                       int32_t B, double* P_out, double* hist_out, double* meta) {
    GD_REQUIRE(ctx && settings && params && cols && P_out && meta && n > 0 && B > 0, "bad argument");
    GD_REQUIRE(ctx->cols, "no samples uploaded");
    GD_REQUIRE(ctx->w_sel == 0, "auxiliary weights are selected");
    GD_HIP(hipSetDevice(ctx->device));
    int rc;
    try {
        std::string err;
        rc = gdb::density1d_batch(state_of(ctx), kOps, kOps1D, ctx, *settings, params, n, cols, B, P_out, hist_out, meta, &err);
        if (rc) ctx->err = err;
    } catch (const std::exception& e) {
        rc = gd_fail(ctx, GD_ERR_NOMEM, "gd_density1d_batch: %s", e.what());
    }
    return rc;
}

int gd_batch2d_finish(gd_ctx* ctx) {
    GD_REQUIRE(ctx, "null context");
    if (!ctx->batch_state) return GD_OK;
    GD_HIP(hipSetDevice(ctx->device));
    return gdb::finish_all(*(gdb::State*)ctx->batch_state, kOps, ctx);
}

int gd_batch2d_exchanges(gd_ctx* ctx, int64_t* count_out) {
    GD_REQUIRE(ctx && count_out, "null argument");
    *count_out = 0;
    if (ctx->batch_state) {
        gdb::State& st = *(gdb::State*)ctx->batch_state;
        std::lock_guard<std::mutex> g(st.mu);
        *count_out = st.exchanges_entered;
    }
    return GD_OK;
}

int gd_batch2d_invalidate(gd_ctx* ctx) {
    GD_REQUIRE(ctx, "null context");
    if (!ctx->batch_state) return GD_OK;
    gdb::invalidate_index_columns(*(gdb::State*)ctx->batch_state);
    return GD_OK;
}

}  // extern "C"
