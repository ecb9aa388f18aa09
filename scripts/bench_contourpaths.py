"""Times the contour paths of the benchmark triangle: the 1225 grids that get2DDensities(get_density=False) returns for the
50 parameters of bench.py's workload, at the grid sizes the batch chooses, two contour levels each.  Same machine, same run;
no threshold.

  (a) the gd_contour_paths call alone over the resident grids (count pass, scan, compaction and ordering, the copy of the
      vertices to page-locked memory): host clock around the blocking call, and device events around the same call;
  (b) the upload of the grids, one copy of the batch's page-locked block;
  (c) MCSamples.get2DContourPaths end to end (densities, levels, upload, paths, result objects), and the get2DDensities
      call it contains by itself;
  (d) when contourpy is importable: its serial algorithm over the same host grids, lines at both levels and the two filled
      bands, one grid after the other on one core -- what ax.contour / ax.contourf do; otherwise null.

    python scripts/bench_contourpaths.py [--nsamples 10000000] [--nparams 50] [--calls 7] [--out profiles/contourpaths_throughput.json]
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
    ap.add_argument("--nsamples", type=int, default=10_000_000)
    ap.add_argument("--nparams", type=int, default=50)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from getdist_amd import synth
    from getdist_amd.contourpaths import _pack_axes, _shared_block, contour_paths
    from getdist_amd.mcsamples import MCSamples

    s, w, names, ranges = synth.config_c3(a.nsamples, a.nparams)
    mc = MCSamples(samples=s, weights=w, names=names, ranges=ranges)
    ctx = mc.ctx
    pairs = synth.triangle_pairs(a.nparams)
    med = lambda t: float(np.median(t))  # noqa: E731
    print("samples resident: %d x %d, %d pairs" % (a.nsamples, a.nparams, len(pairs)), flush=True)

    dens = list(mc.get2DDensities(pairs, num_plot_contours=2, get_density=False))
    grids = [d.P for d in dens]
    levels = np.array([d.contours for d in dens])
    shared = _shared_block(grids)  # the batch's own page-locked block
    assert shared is not None, "the grids of one batched call share a block"
    block, offs = shared
    ny, nx = [g.shape[0] for g in grids], [g.shape[1] for g in grids]
    (xs, x_off), (ys, y_off) = _pack_axes([d.x for d in dens]), _pack_axes([d.y for d in dens])
    sizes = {}
    for g in grids:
        sizes[g.shape[0]] = sizes.get(g.shape[0], 0) + 1
    res = dict(nsamples=a.nsamples, nparams=a.nparams, grids=len(grids), levels_per_grid=int(levels.shape[1]), calls=a.calls,
               warmup=a.warmup, axis_doubles=int(xs.size + ys.size), grid_sizes={str(k): v for k, v in sorted(sizes.items())}, grid_bytes=int(block.nbytes))

    dev = ctx.alloc(block.nbytes)
    t_up = timed(lambda: dev.from_host(block), a.warmup + a.calls)[a.warmup:]

    def call():
        return ctx.contour_paths(dev, offs, ny, nx, xs, x_off, ys, y_off, levels)

    for _ in range(a.warmup):
        out = call()
    t_call = timed(call, a.calls)
    t_dev = []
    for _ in range(a.calls):
        ctx.timer_start()
        out = call()
        t_dev.append(ctx.timer_stop_ms())
    xy, flag, loops, voff, loff, status = out
    assert not status.any()
    res.update(vertices=int(voff[-1]), loops=int(loff[-1]), result_bytes=int(xy.nbytes + flag.nbytes + loops.nbytes),
               upload_ms=t_up, upload_ms_median=med(t_up), upload_GBps=block.nbytes / 1e6 / med(t_up),
               native_call_ms=t_call, native_call_ms_median=med(t_call), native_call_device_ms=t_dev,
               native_call_device_ms_median=med(t_dev))
    dev.free()
    print("(a) gd_contour_paths: %.2f ms per call (device events %.2f ms), %d vertices in %d loops, %.1f MB of results\n"
          "(b) upload of %.0f MB of grids: %.2f ms (%.1f GB/s)"
          % (med(t_call), med(t_dev), voff[-1], loff[-1], res["result_bytes"] / 1e6, block.nbytes / 1e6, med(t_up),
             res["upload_GBps"]), flush=True)

    for _ in range(a.warmup):
        mc.get2DContourPaths(pairs, num_plot_contours=2)
    t_e2e = timed(lambda: mc.get2DContourPaths(pairs, num_plot_contours=2), a.calls)
    t_dens = timed(lambda: list(mc.get2DDensities(pairs, num_plot_contours=2, get_density=False)), a.calls)
    res.update(get2DContourPaths_ms=t_e2e, get2DContourPaths_ms_median=med(t_e2e), get2DDensities_levels_ms=t_dens,
               get2DDensities_levels_ms_median=med(t_dens), end_to_end_minus_densities_ms=med(t_e2e) - med(t_dens))
    print("(c) get2DContourPaths end to end: %.1f ms; get2DDensities(get_density=False) alone: %.1f ms"
          % (med(t_e2e), med(t_dens)), flush=True)

    res.update(contourpy_version=None, contourpy_ms=None, contourpy_lines_ms=None, contourpy_filled_ms=None,
               native_call_speedup_over_contourpy=None, same_line_counts_as_contourpy=None)
    try:
        import contourpy
    except ImportError:
        contourpy = None
    if contourpy is not None:
        t_lines = t_filled = 0.0
        same = True
        got = contour_paths(dens, ctx=ctx)  # of the very grids contourpy gets
        for k, d in enumerate(dens):
            gen = contourpy.contour_generator(d.x, d.y, d.P, name="serial")
            lv = sorted(float(v) for v in d.contours)
            t0 = time.perf_counter()
            lines = [gen.lines(v) for v in lv]
            t1 = time.perf_counter()
            for lo, hi in zip(lv, lv[1:] + [np.inf]):
                gen.filled(lo, hi)
            t2 = time.perf_counter()
            t_lines += t1 - t0
            t_filled += t2 - t1
            if k % 25 == 0:  # faster and different is not faster: the same lines, by count
                order = np.argsort(d.contours)
                for q, ref in zip(order, lines):
                    mine = got[k].lines(int(q))
                    same = same and sorted(len(m) for m in mine) == sorted(len(r) for r in ref)
        total = (t_lines + t_filled) * 1e3
        res.update(contourpy_version=contourpy.__version__, contourpy_ms=total, contourpy_lines_ms=t_lines * 1e3,
                   contourpy_filled_ms=t_filled * 1e3, native_call_speedup_over_contourpy=total / med(t_call),
                   same_line_counts_as_contourpy=bool(same))
        print("(d) contourpy %s on one core: lines %.0f ms + filled bands %.0f ms = %.0f ms, %.0f x the native call; same line "
              "counts on every 25th grid: %s" % (contourpy.__version__, t_lines * 1e3, t_filled * 1e3, total, total / med(t_call), same),
              flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python " + " ".join(sys.argv), result=res), f, indent=1)
    if res["same_line_counts_as_contourpy"] is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
