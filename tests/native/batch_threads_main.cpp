// Stand-alone thread test of gd_density2d_batch's choreography (getdist_amd/csrc/batch2d.hpp): the table of device entry
// points bound to C++ stubs -- no Python, no numerics -- so that the hand-offs between the call's threads run under
// ThreadSanitizer and AddressSanitizer as a plain executable (tests/native/build_threads.py, tests/test_batch_threads.py).
//
//   batch_threads_main list          the names of the runs, one per line
//   batch_threads_main <run>         one run; exit status 0 = passed
//
// "shapes": four shapes of a call, twice each on one state (the second finds the pool and the index columns filled).
// Every other run repeats the last shape -- staged, deferred chain, two binning launches -- on a fresh state with one
// fault: the n-th call of one stub returns GD_ERR_HIP or throws std::bad_alloc.  The call must come back with a non-zero
// code, and every block the stubs handed out must be freed once the state is released.  A run that does not end is the
// failure this program exists for: the caller gives each run a time limit.
#include <new>

#include "../../getdist_amd/csrc/batch2d.hpp"

namespace {

constexpr int kParams = 13;
constexpr int64_t kRows = 1000;
constexpr int64_t kItem = 65536 * 8;  // bytes of a base-grid histogram

struct Ctx {
    int id;
};

// ---- fault injection and block accounting -----------------------------------------------------------------------------
struct Fault {
    const char* name;
    const char* op;
    int nth;
    bool throws;
    int64_t bytes;  // dev_alloc only: the size that counts (0: any)
};
const Fault* g_fault = nullptr;
std::atomic<int> g_hits{0};
std::atomic<bool> g_fired{false};

int hit(const char* op, int64_t bytes = 0) {
    const Fault* f = g_fault;
    if (!f || strcmp(f->op, op) != 0 || (f->bytes && f->bytes != bytes)) return 0;
    if (++g_hits != f->nth) return 0;
    g_fired = true;
    if (f->throws) throw std::bad_alloc();
    return GD_ERR_HIP;
}

std::mutex g_mu;
std::map<void*, int64_t> g_blocks;
int g_aux_live = 0;
std::atomic<int> g_marks{0}, g_waits{0};

double* last_double(void* p, int64_t bytes) { return (double*)((char*)p + bytes - 8); }
void touch(void* p, int64_t bytes) { *(double*)p = 1.0, *last_double(p, bytes) = 1.0; }

gdb::Ops make_ops() {
    gdb::Ops o;
    memset(&o, 0, sizeof o);
    o.bind_thread = [](void*) { return 0; };
    o.num_rows = [](void*, int64_t* N, int64_t* n) {
        *N = kRows, *n = kParams;
        return 0;
    };
    o.weights_kind = [](void*, int32_t* hw) {
        *hw = 0;
        return 0;
    };
    o.dev_alloc = [](void*, int64_t bytes, void** out) {
        if (int e = hit("dev_alloc", bytes)) return e;
        void* p = malloc((size_t)bytes);
        if (!p) return (int)GD_ERR_NOMEM;
        std::lock_guard<std::mutex> g(g_mu);
        g_blocks[p] = bytes;
        *out = p;
        return 0;
    };
    o.dev_free = [](void*, void* p) {
        std::lock_guard<std::mutex> g(g_mu);
        if (!g_blocks.erase(p)) {
            fprintf(stderr, "dev_free of a block that is not out\n");
            abort();
        }
        free(p);
        return 0;
    };
    o.prebin8_batch = [](void*, const int32_t*, int32_t ncols, const double*, const double*, int32_t, void* const* d_idx, int64_t* bad) {
        for (int q = 0; q < ncols; ++q) ((uint8_t*)d_idx[q])[kRows - 1] = 1, bad[q] = 0;
        return 0;
    };
    o.hist2d_prebinned8 = [](void*, int32_t B, const void* const*, const void* const*, void* d_hist) {
        if (int e = hit("hist2d_prebinned8")) return e;
        touch(d_hist, B * kItem);
        return 0;
    };
    o.prebin8_hist2d = [](void*, const int32_t*, int32_t ncols, const double*, const double*, void* const* d_idx, int64_t* bad, int32_t B,
                          const void* const*, const void* const*, void* d_hist) {
        if (int e = hit("prebin8_hist2d")) return e;
        for (int q = 0; q < ncols; ++q) ((uint8_t*)d_idx[q])[kRows - 1] = 1, bad[q] = 0;
        touch(d_hist, B * kItem);
        return 0;
    };
    o.prebin = [](void*, int32_t, double, double, int32_t, void* d_idx) {
        ((uint16_t*)d_idx)[kRows - 1] = 1;
        return 0;
    };
    o.prebin_batch = [](void*, const int32_t*, int32_t ncols, const double*, const double*, int32_t, void* const* d_idx) {
        for (int q = 0; q < ncols; ++q) ((uint16_t*)d_idx[q])[kRows - 1] = 1;
        return 0;
    };
    o.hist2d_prebinned = [](void*, int32_t B, const void* const*, const void* const*, int32_t F, void* d_hist) {
        touch(d_hist, (int64_t)B * F * F * 8);
        return 0;
    };
    o.minmax_affine = [](void*, int32_t B, const int32_t*, const int32_t*, const double*, const double*, double* out) {
        for (int q = 0; q < B; ++q) out[2 * q] = 0.0, out[2 * q + 1] = 1.0;
        return 0;
    };
    o.hist2d_sheared = [](void*, int32_t B, const int32_t*, const int32_t*, const double*, const double*, const double*, const double*,
                          const double*, const double*, int32_t F, void* d_hist) {
        if (int e = hit("hist2d_sheared")) return e;
        touch(d_hist, (int64_t)B * F * F * 8);
        return 0;
    };
    static const auto rows = [](int32_t B, double* out) {
        for (int q = 0; q < B; ++q) {
            double* o = out + (size_t)q * 12;
            for (int c = 0; c < 12; ++c) o[c] = 0.5;
            o[7] = 0, o[8] = 0.05, o[9] = 0.04, o[10] = 0.1, o[11] = 0;
        }
    };
    o.kopt2d = [](void*, int32_t B, int32_t, const void*, const double*, const int32_t*, const double*, const double*, double* out) {
        rows(B, out);
        return 0;
    };
    o.gather_items = [](void*, void* d_dst, int64_t dst_first, const void*, const int32_t*, int32_t count, int64_t item_bytes) {
        touch((char*)d_dst + dst_first * item_bytes, count * item_bytes);
        return 0;
    };
    o.density2d_enqueue = [](void*, int32_t B, int32_t F, const void*, const int32_t*, const double*, const double*, const double*,
                             const int32_t*, const int32_t*, int32_t, int32_t, void* d_P, int32_t* status) {
        if (int e = hit("density2d_enqueue")) return e;
        touch(d_P, (int64_t)B * F * F * 8);
        for (int q = 0; q < B; ++q) status[q] = 0;
        return 0;
    };
    o.d2h_async = [](void*, void* dst, const void* d_src, int64_t bytes) {
        *(double*)dst = *(const double*)d_src;
        *last_double(dst, bytes) = *last_double((void*)d_src, bytes);
        return 0;
    };
    o.copy_mark = [](void*, int32_t* token) {
        *token = ++g_marks;
        return 0;
    };
    o.copy_wait = [](void*, int32_t) {
        ++g_waits;
        return 0;
    };
    o.copy_sync = [](void*) { return 0; };
    o.autocov_lags_batch = [](void*, const int32_t*, int32_t ncols, const double*, int64_t, int32_t nlags, double* out) {
        for (int q = 0; q < ncols * nlags; ++q) out[q] = q % nlags ? 0.0 : 0.01 * kRows;  // uncorrelated at lag 1
        return 0;
    };
    o.kde_lag_sums_batch = [](void*, const int32_t*, int32_t ncols, const double*, const int64_t*, int32_t nlags, double* out) {
        for (int q = 0; q < ncols * nlags; ++q) out[q] = 0.0;
        return 0;
    };
    o.kde_lag_sums = [](void*, int32_t, double, const int64_t*, int32_t nlags, double* out) {
        for (int q = 0; q < nlags; ++q) out[q] = 0.0;
        return 0;
    };
    o.last_error = [](void*) -> const char* { return "a stub failed"; };
    o.create_aux = [](void*, void** aux) {
        std::lock_guard<std::mutex> g(g_mu);
        *aux = new Ctx{100 + g_aux_live++};
        return 0;
    };
    o.destroy_aux = [](void* aux) {
        std::lock_guard<std::mutex> g(g_mu);
        delete (Ctx*)aux;
        --g_aux_live;
        return 0;
    };
    o.kopt2d_enqueue = [](void*, int32_t, int32_t, const void*, const double*, const int32_t*, const double*, const double*, void*,
                          int32_t* ticket) {
        if (int e = hit("kopt2d_enqueue")) return e;
        *ticket = 1;
        return 0;
    };
    o.kopt2d_finish = [](void*, void*, int32_t, int32_t B, void* d_rows, double* out) {
        if (int e = hit("kopt2d_finish")) return e;
        touch(d_rows, (int64_t)B * GD_KOPT_BLOCK_DOUBLES * 8);
        rows(B, out);
        return 0;
    };
    return o;
}

// ---- the problem: a triangle of 13 parameters ---------------------------------------------------------------------------
// Pairs with (i + j) % 3 == 0 are correlated (0.5: sheared, branch A), the others are not (the optimiser's own, branch C);
// two pairs at 0.95 are sheared on an up-scaled grid and one at 0.995 takes the rule of thumb on the largest grid: three
// grid-size classes, of which the deferred chain bins two.
struct Problem {
    gd_batch2d_settings s;
    std::vector<gd_param2d> par;
    std::vector<double> corr, cov;
    std::vector<int32_t> pairs;
    int nA = 0, nC = 0;  // among the pairs of the base grid
    std::vector<double> grids, meta;
    std::vector<int32_t> status;

    Problem() : par(kParams), corr(kParams * kParams, 0.0), cov(kParams * kParams, 0.0) {
        memset(&s, 0, sizeof s);
        s.fine_bins_2D = 256, s.boundary_correction_order = 1, s.mult_bias_correction_order = 1, s.num_bins_2D = 40;
        s.smooth_scale_2D = -1.0, s.max_corr_2D = 0.99, s.norm = (double)kRows, s.sum_w2 = (double)kRows;
        s.two_streams_min = 8, s.two_streams_split = 20, s.kopt_split_min = 8;  // (78 pairs take the routes of a full triangle)
        for (int j = 0; j < kParams; ++j) {
            gd_param2d& p = par[j];
            memset(&p, 0, sizeof p);
            p.range_min = 0.05, p.range_max = 0.95, p.param_min = 0.0, p.param_max = 1.0, p.sigma_range = 0.1, p.err = 0.1;
            p.mean = 0.5, p.var = 0.01, p.neff = NAN, p.owned = 1;
        }
        for (int i = 0; i < kParams; ++i)
            for (int j = 0; j < kParams; ++j) {
                double c = i == j ? 1.0 : ((i + j) % 3 == 0 ? 0.5 : 0.0);
                const int a = std::min(i, j), b = std::max(i, j);
                if ((a == 0 && b == 1) || (a == 2 && b == 3)) c = 0.95;
                if (a == 4 && b == 5) c = 0.995;
                corr[i * kParams + j] = c, cov[i * kParams + j] = c * 0.01;
            }
        for (int i = 0; i < kParams; ++i)
            for (int j = i + 1; j < kParams; ++j) {
                pairs.push_back(i), pairs.push_back(j);
                const double c = corr[i * kParams + j];
                nA += c == 0.5, nC += c == 0.0;
            }
    }
    void buffers() {  // (75 grids of 256^2, two of 576^2, one of 960^2)
        const size_t P = pairs.size() / 2;
        grids.resize(P * 65536 + 2 * 576 * 576 + 960 * 960), meta.resize(P * GD_BATCH2D_META), status.resize(P);
    }
    void forget_neff() {
        for (gd_param2d& p : par) p.neff = NAN;
    }
};

const gdb::Ops kOps = make_ops();
Ctx g_main{1}, g_twin{2};

int call(gdb::State& st, Problem& pb, int P, bool with_twin, std::string* err) {
    int32_t tokens[2];
    if (pb.grids.empty()) pb.buffers();
    gdb::Call c(st, kOps, &g_main, with_twin ? &g_twin : nullptr, pb.s, pb.par.data(), kParams, pb.corr.data(), pb.cov.data(), nullptr,
                pb.pairs.data(), P, nullptr, nullptr, pb.grids.data(), (int64_t)pb.grids.size(), pb.status.data(), pb.meta.data(),
                nullptr, nullptr);
    try {  // (as the library's entry does: the stack is unwound, the call's threads are waited for)
        const int rc = c.run(tokens);
        *err = c.err;
        return rc;
    } catch (const std::exception& e) {
        *err = e.what();
        return -99;
    }
}

// every block back, every context gone, once the state is released
bool released_clean(gdb::State& st) {
    gdb::release_all(st, kOps, &g_main);
    std::lock_guard<std::mutex> g(g_mu);
    if (!g_blocks.empty() || g_aux_live != 0) {
        fprintf(stderr, "after release: %zu blocks out, %d contexts alive\n", g_blocks.size(), g_aux_live);
        return false;
    }
    return true;
}

void deferred_chain(bool on) {
    setenv("GDHIP_BATCH_SHEAR_DEFERRED_MIN", "16", 1);
    setenv("GDHIP_BATCH_SHEAR_DEFERRED", on ? "1" : "0", 1);
}

bool run_shapes() {
    Problem pb;
    const int P = (int)pb.pairs.size() / 2;
    gdb::State st;
    struct Shape {
        const char* name;
        int P;
        bool twin, deferred;
    } shapes[] = {{"small sequential", 10, false, true}, {"two streams", 30, true, true}, {"staged", P, true, false},
                  {"staged, deferred chain, two binning launches", P, true, true}};
    for (const Shape& sh : shapes)
        for (int round = 0; round < 2; ++round) {
            deferred_chain(sh.deferred);
            if (round == 0) pb.forget_neff();
            pb.s.results_in_flight = round;
            for (int32_t& w : pb.status) w = -7;
            std::string err;
            const int rc = call(st, pb, sh.P, sh.twin, &err);
            if (rc) {
                fprintf(stderr, "%s, call %d: rc %d (%s)\n", sh.name, round, rc, err.c_str());
                return false;
            }
            for (int k = 0; k < sh.P; ++k) {
                const double* m = &pb.meta[(size_t)k * GD_BATCH2D_META];
                if (pb.status[(int)m[30]] != 0 || !(m[2] > 0) || !(m[3] > 0) || !(m[21] >= 1)) {
                    fprintf(stderr, "%s, call %d: pair %d was not delivered\n", sh.name, round, k);
                    return false;
                }
            }
        }
    if (g_marks == 0 || g_waits == 0) {
        fprintf(stderr, "no result copy was marked or waited for\n");
        return false;
    }
    return released_clean(st);
}

std::vector<Fault> faults(const Problem& pb) {
    // the first optimiser part of the last shape: half of the base grid's optimiser and sheared pairs, gathered into a block of its own
    const int64_t first_part = std::max<int64_t>(8, (pb.nC + pb.nA + 1) / 2);
    std::vector<Fault> f;
    for (int t = 0; t < 2; ++t) {
        const bool th = t == 1;
        f.push_back({th ? "fused-binning-throws" : "fused-binning-fails", "prebin8_hist2d", 1, th, 0});
        f.push_back({th ? "second-binning-throws" : "second-binning-fails", "hist2d_prebinned8", 1, th, 0});
        f.push_back({th ? "sheared-histograms-throw" : "sheared-histograms-fail", "hist2d_sheared", 1, th, 0});
        f.push_back({th ? "second-stage-a-throws" : "second-stage-a-fails", "kopt2d_enqueue", 2, th, 0});
        f.push_back({th ? "first-get-h-throws" : "first-get-h-fails", "kopt2d_finish", 1, th, 0});
        f.push_back({th ? "convolution-throws" : "convolution-fails", "density2d_enqueue", 1, th, 0});
        f.push_back({th ? "build-batch-alloc-throws" : "build-batch-alloc-fails", "dev_alloc", 1, th, first_part * kItem});
    }
    return f;
}

bool run_fault(const Fault& f) {
    Problem pb;
    gdb::State st;
    deferred_chain(true);
    g_hits = 0, g_fired = false, g_fault = &f;
    std::string err;
    const int rc = call(st, pb, (int)pb.pairs.size() / 2, true, &err);
    g_fault = nullptr;
    if (!g_fired) {
        fprintf(stderr, "%s: the fault was never reached\n", f.name);
        return false;
    }
    if (rc == 0) {
        fprintf(stderr, "%s: the call returned 0\n", f.name);
        return false;
    }
    return released_clean(st);
}

}  // namespace

int main(int argc, char** argv) {
    const Problem pb;
    const std::vector<Fault> fs = faults(pb);
    const std::string run = argc > 1 ? argv[1] : "list";
    if (run == "list") {
        printf("shapes\n");
        for (const Fault& f : fs) printf("%s\n", f.name);
        return 0;
    }
    bool ok = false, found = run == "shapes";
    if (found) ok = run_shapes();
    for (const Fault& f : fs)
        if (run == f.name) found = true, ok = run_fault(f);
    if (!found) {
        fprintf(stderr, "no such run: %s\n", run.c_str());
        return 2;
    }
    printf("%s: %s\n", run.c_str(), ok ? "passed" : "FAILED");
    return ok ? 0 : 1;
}
