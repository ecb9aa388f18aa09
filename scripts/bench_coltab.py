"""Times the table look-ups of column expressions at 1e7 x 50 unit-weight fp64 rows (4 GB resident): np.interp over 1 000
knots, a Density1D.Prob over 1 000 knots and a Density2D.Prob over 128 x 128 coefficients.  Same machine, same run; no
threshold.

  (a) the gd_expr_eval_tab call alone for one INTERP, one SPLINE1 and one SPLINE2 into a spare column (reads one or two
      columns, writes one; device events around table copy, launch and wait), and the host clock of the same call;
  (b) the derived vector placed in a spare column by the expression (np.interp(p.x, ...) evaluated on the device) and
      samples.addDerived(np.interp(p.x, ...)) end to end, once;
  (c) the host route: the host column through np.interp / Density1D.Prob / RectBivariateSpline.ev, then the N-vector
      uploaded into the spare column; and addDerived of the numpy-built vector, once;
  (d) a device-to-device copy moving as many bytes as the one-column look-ups read and write, as the streaming roof.

    python scripts/bench_coltab.py [--rows 10000000] [--cols 50] [--calls 7] [--out profiles/coltab_throughput.json]

The comparison without LDS staging of the knots (profiles/coltab_throughput_nostaging.json): build a second library,

    GDHIP_EXTRA_FLAGS=-DGD_TAB_NO_STAGING bash getdist_amd/csrc/build.sh build/nostaging

and run with --lib build/nostaging/libgdhip.so --note "built with -DGD_TAB_NO_STAGING".
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
    ap.add_argument("--lib", default=None, help="a libgdhip.so to load instead of the tree's")
    ap.add_argument("--note", default="", help="kept in the result, e.g. how the library was built")
    a = ap.parse_args()
    from getdist_amd import _lib

    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from getdist_amd.densities import Density1D, Density2D
    from getdist_amd.mcsamples import MCSamples

    names = ["p%d" % j for j in range(a.cols)]
    names[3], names[17] = "x", "y"
    samples = np.random.default_rng(20261020).random((a.cols, a.rows)).T  # (rows, cols), column-major; x, y in [0, 1)
    print("samples: %d x %d, %.2f GB" % (a.rows, a.cols, samples.nbytes / 1e9), flush=True)
    s = MCSamples(samples=samples, names=names)
    ctx = s.ctx
    print("resident", flush=True)

    rng = np.random.default_rng(5)
    zgrid = np.sort(rng.uniform(0.05, 0.95, 1000))  # irregular knots; some rows fall outside
    dgrid = np.sqrt(zgrid) + 0.01 * rng.standard_normal(1000)
    g1 = np.linspace(0.02, 0.98, 1000)
    d1 = Density1D(g1, np.exp(-0.5 * ((g1 - 0.5) / 0.2) ** 2))
    g2 = np.linspace(0.02, 0.98, 128)
    d2 = Density2D(g2, g2, np.exp(-0.5 * (((g2[None, :] - 0.5) / 0.2) ** 2 + ((g2[:, None] - 0.4) / 0.3) ** 2)))
    build = {"interp": lambda p: np.interp(p.x, zgrid, dgrid), "spline1": lambda p: d1.Prob(p.x),
             "spline2": lambda p: d2.Prob(p.x, p.y)}
    p, h = s.getDeviceParams(), s.getParams()
    med = lambda t: float(np.median(t))  # noqa: E731
    res = dict(rows=a.rows, cols=a.cols, weights="unit", calls=a.calls, note=a.note, tables=dict(interp="1000 knots", spline1="1000 knots",
                                                                                      spline2="128 x 128 coefficients"))

    src, dst = ctx.alloc(a.rows * 8), ctx.alloc(a.rows * 8)
    ctx._check(ctx.lib.gd_memset(ctx.h, src.ptr, 1, src.nbytes))

    def d2d():
        ctx.timer_start()
        ctx.copy_d2d(dst, 0, src, 0, src.nbytes)
        return ctx.timer_stop_ms()

    same = True
    for name, fn in build.items():
        expr = fn(p)
        code, consts, tables = expr.compile_with_tables(s)
        nbytes = len(code) * a.rows * 8  # one column read per COL step, one written

        def call():
            ctx.timer_start()
            ctx.expr_eval(code, consts, _lib.GD_EX_TO_COLUMN, 0, tables=tables)
            return ctx.timer_stop_ms()

        call(), d2d()
        t_call, t_d2d = [], []
        for _ in range(a.calls):  # interleaved: both see the same clocks
            t_call.append(call())
            t_d2d.append(d2d())
        t_wall = timed(lambda: ctx.expr_eval(code, consts, _lib.GD_EX_TO_COLUMN, 0, tables=tables), a.calls)

        def host_route():
            with np.errstate(all="ignore"):
                ctx.set_extra_column(1, fn(h))

        host_route()
        t_host = timed(host_route, a.calls)
        with np.errstate(all="ignore"):
            want = fn(h)
        got = expr.eval(s)
        ok = bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))
        same = same and ok
        res[name] = dict(bytes=nbytes, call_ms=t_call, call_ms_median=med(t_call), call_GBps=nbytes / 1e6 / med(t_call),
                         call_wall_ms=t_wall, call_wall_ms_median=med(t_wall), d2d_ms=t_d2d, d2d_ms_median=med(t_d2d),
                         d2d_GBps=2 * a.rows * 8 / 1e6 / med(t_d2d), host_route_ms=t_host, host_route_ms_median=med(t_host),
                         bit_equal_to_host=ok)
        print("%-8s (a) call %.3f ms (%.0f GB/s of %d MB; host clock %.3f ms)  (c) host route %.1f ms  (d) copy of 160 MB %.3f ms  "
              "bit-equal: %s" % (name, med(t_call), res[name]["call_GBps"], nbytes // 10**6, med(t_wall), med(t_host), med(t_d2d), ok),
              flush=True)
    src.free(), dst.free()

    # (b) / (c) end to end, once each: addDerived re-uploads the sample set, which both routes pay alike
    t0 = time.perf_counter()
    s.addDerived(np.interp(p.x, zgrid, dgrid), "DA")
    t_add_expr = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    s.addDerived(np.interp(s.getParams().x, zgrid, dgrid), "DA_host")
    t_add_host = (time.perf_counter() - t0) * 1e3
    ok = bool(np.array_equal(s.samples[:, -1].view(np.uint64), s.samples[:, -2].view(np.uint64)))
    same = same and ok
    res.update(addDerived_expr_ms=t_add_expr, addDerived_host_ms=t_add_host, addDerived_bit_equal=ok, results_bit_equal=same)
    print("(b) addDerived(np.interp(expr)) %.0f ms  (c) addDerived(np.interp(host column)) %.0f ms  bit-equal: %s"
          % (t_add_expr, t_add_host, ok))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python " + " ".join(sys.argv), result=res), f, indent=1)  # the command as it was given
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
