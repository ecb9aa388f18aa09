"""Times a column expression at 1e7 x 50 unit-weight fp64 rows (4 GB resident): S8 = sigma8 * sqrt(omegam / 0.3) under the
mask (H0 > 70) & (omegam < 0.3).  Same machine, same run; no threshold.

  (a) the kernel alone: gd_expr_eval of S8 into a spare column (reads two columns, writes one);
  (b) samples.mean(S8, where=mask) end to end with expressions (two gd_expr_eval launches and one gd_cov);
  (c) the host route, the same call given the numpy-built vector and mask -- numpy's temporaries, then two N-vectors over
      PCIe: the code path before expressions existed;
  (d) a device-to-device copy moving as many bytes as (a) reads and writes, as the streaming roof.

    python scripts/bench_colexpr.py [--rows 10000000] [--cols 50] [--calls 7] [--out profiles/colexpr_throughput.json]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=50)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from getdist_amd import _lib
    from getdist_amd.mcsamples import MCSamples

    names = ["p%d" % j for j in range(a.cols)]
    names[3], names[17], names[31] = "omegam", "sigma8", "H0"
    samples = np.random.default_rng(20261020).random((a.cols, a.rows)).T  # (rows, cols), column-major
    samples[:, 3] = 0.2 + 0.2 * samples[:, 3]
    samples[:, 17] = 0.7 + 0.2 * samples[:, 17]
    samples[:, 31] = 60.0 + 20.0 * samples[:, 31]
    print("samples: %d x %d, %.2f GB" % (a.rows, a.cols, samples.nbytes / 1e9), flush=True)
    s = MCSamples(samples=samples, names=names)
    ctx = s.ctx
    print("resident", flush=True)

    def build(p):
        return p.sigma8 * np.sqrt(p.omegam / 0.3), (p.H0 > 70) & (p.omegam < 0.3)

    expr, mask = build(s.getDeviceParams())
    code, consts = expr.compile(s)
    kernel_bytes = 3 * a.rows * 8  # two columns read, one written

    def kernel():  # device time of the launch (events on the context's stream)
        ctx.timer_start()
        ctx.expr_eval(code, consts, _lib.GD_EX_TO_COLUMN, 0)
        return ctx.timer_stop_ms()

    src, dst = ctx.alloc(kernel_bytes // 2), ctx.alloc(kernel_bytes // 2)
    ctx._check(ctx.lib.gd_memset(ctx.h, src.ptr, 1, src.nbytes))

    def d2d():
        ctx.timer_start()
        ctx.copy_d2d(dst, 0, src, 0, src.nbytes)
        return ctx.timer_stop_ms()

    kernel(), d2d()  # warm-up
    t_kernel, t_d2d = [], []
    for _ in range(a.calls):  # interleaved: both see the same clocks
        t_kernel.append(kernel())
        t_d2d.append(d2d())
    t_kernel_wall = timed(lambda: ctx.expr_eval(code, consts, _lib.GD_EX_TO_COLUMN, 0), a.calls)
    src.free(), dst.free()
    print("kernel and copy done", flush=True)

    got = []
    s.mean(expr, where=mask)
    t_expr = timed(lambda: got.append(s.mean(expr, where=mask)), a.calls)
    print("expression route done", flush=True)

    want = []

    def host_route():
        vec, m = build(s.getParams())
        want.append(s.mean(vec, where=m))

    host_route()
    t_host = timed(host_route, a.calls)
    t_numpy = timed(lambda: build(s.getParams()), a.calls)  # the share of (c) that is numpy arithmetic
    same = all(g == w for g, w in zip(got, want[1:]))

    med = lambda t: float(np.median(t))  # noqa: E731
    res = dict(rows=a.rows, cols=a.cols, weights="unit", calls=a.calls, expression="sigma8*sqrt(omegam/0.3)",
               mask="(H0 > 70) & (omegam < 0.3)", kernel_bytes=kernel_bytes,
               kernel_ms=t_kernel, kernel_ms_median=med(t_kernel), kernel_GBps=kernel_bytes / 1e6 / med(t_kernel),
               kernel_call_wall_ms=t_kernel_wall, kernel_call_wall_ms_median=med(t_kernel_wall),
               d2d_ms=t_d2d, d2d_ms_median=med(t_d2d), d2d_GBps=kernel_bytes / 1e6 / med(t_d2d),
               kernel_bytes_at_d2d_rate_ms=kernel_bytes / (kernel_bytes / med(t_d2d)),  # (a)'s bytes over (d)'s rate
               kernel_over_d2d_rate=med(t_d2d) / med(t_kernel),
               mean_expr_ms=t_expr, mean_expr_ms_median=med(t_expr),
               mean_host_ms=t_host, mean_host_ms_median=med(t_host),
               host_numpy_ms=t_numpy, host_numpy_ms_median=med(t_numpy),
               results_bit_equal=bool(same), mean=float(got[0]))
    print("(a) kernel %.3f ms (%.0f GB/s of %d MB)  (d) device copy of the same bytes %.3f ms (%.0f GB/s): kernel at %.2f of "
          "the copy's rate\n(b) mean(expr, where=mask) %.2f ms  (c) host route %.1f ms, of which numpy %.1f ms; medians of %d calls"
          % (res["kernel_ms_median"], res["kernel_GBps"], kernel_bytes // 10**6, res["d2d_ms_median"], res["d2d_GBps"],
             res["kernel_over_d2d_rate"], res["mean_expr_ms_median"], res["mean_host_ms_median"], res["host_numpy_ms_median"],
             a.calls))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python " + " ".join(sys.argv), result=res), f, indent=1)  # the command as it was given
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
