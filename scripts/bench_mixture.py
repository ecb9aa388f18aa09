"""Times gd_mixture_nll at the headline shape (the C3 block of synth.config_c3: N = 1e7 rows, d = 50 columns, K = 3
components) and prints, next to it, the HBM floor of one read of the columns and the numpy einsum time of the host
alternative (MixtureND.pdf) on the same machine.

    python scripts/bench_mixture.py [--rows 10000000] [--launches 20] [--warmup 3] [--no-numpy]

The per-call figure is the context's event timer around the whole entry (kernel + the D2H of the N-double result); the
kernel alone comes from a kernel trace of the same script (rocprofv3 --kernel-trace --stats -- python scripts/bench_mixture.py
--no-numpy), D2H = call - kernel."""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0  # bench.py's figure (MI355X spec; about 6300 GB/s achievable)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    from getdist_amd import gaussian_mixtures as gm
    from getdist_amd import synth
    from getdist_amd._lib import Context

    d, K = 50, 3
    s, _, names, _ = synth.config_c3(a.rows, d)
    r = np.random.default_rng(1)
    base = np.cov(s[:200_000].T)
    mean = s[:200_000].mean(axis=0)
    mix = gm.MixtureND([mean + 0.2 * k * np.sqrt(np.diag(base)) for k in range(K)], [base * (1 + 0.3 * k) for k in range(K)],
                       r.uniform(0.5, 1.5, K), names=names)
    whiten, logcoef = mix._whitened()
    ctx = Context(0)
    ctx.upload(s)
    cols = list(range(d))
    for _ in range(a.warmup):
        out = ctx.mixture_nll(cols, mix.means, whiten, logcoef)
    ms, wall = [], []
    for _ in range(a.launches):
        t0 = time.perf_counter()
        ctx.timer_start()
        out = ctx.mixture_nll(cols, mix.means, whiten, logcoef)
        ms.append(ctx.timer_stop_ms())
        wall.append((time.perf_counter() - t0) * 1e3)
    ms, wall = np.array(ms), np.array(wall)
    bytes_read = a.rows * d * 8.0
    fma = a.rows * K * d * (d + 1) / 2.0
    print("gd_mixture_nll N=%d d=%d K=%d: call (kernel + D2H) median %.3f ms (min %.3f, max %.3f; host clock median %.3f) "
          "over %d launches after %d warm-ups" % (a.rows, d, K, np.median(ms), ms.min(), ms.max(), np.median(wall), a.launches,
                                                  a.warmup))
    print("  one read of the columns: %.3f GB -> %.3f ms at %.0f GB/s (HBM peak), %.3f ms at 6300 GB/s"
          % (bytes_read / 1e9, bytes_read / HBM_PEAK_GBS / 1e6, HBM_PEAK_GBS, bytes_read / 6300.0 / 1e6))
    print("  fp64 FMAs: %.3e (%.3e flop) -> %.3f ms at 78.6 Tflop/s (fp64 vector peak)" % (fma, 2 * fma, 2 * fma / 78.6e12 * 1e3))
    print("  result D2H: %.3f GB" % (a.rows * 8.0 / 1e9))
    if not a.no_numpy:
        t0 = time.perf_counter()
        with np.errstate(divide="ignore"):
            host = -np.log(mix.pdf(s))
        t_np = time.perf_counter() - t0
        ok = np.isfinite(host)
        print("  numpy einsum (-log(MixtureND.pdf(rows)), the host alternative): %.2f s; max |device - numpy| %.3e over the %d "
              "rows where numpy is finite" % (t_np, float(np.max(np.abs(np.asarray(out)[ok] - host[ok]))), int(ok.sum())))
    ctx.close()


if __name__ == "__main__":
    main()
