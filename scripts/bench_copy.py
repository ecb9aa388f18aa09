"""Times MCSamples.copy at 1e7 x 50 unit-weight fp64 rows (4 GB resident): the whole call (host state deep-copied, the
resident columns cloned device to device), the gd_clone_samples call alone into a fresh context, and -- what a copy would
cost without it -- Context.upload of the same host array into a fresh context.  Same machine, same run; no threshold.

    python scripts/bench_copy.py [--rows 10000000] [--cols 50] [--calls 5] [--out profiles/copy_clone.json]

The host array is column-major, the layout the upload takes without a transpose (its fastest route)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls, before=None, after=None):
    """Milliseconds of ``fn(before())`` per call; ``after(result)`` cleans up outside the timed region."""
    out = []
    for _ in range(calls):
        arg = before() if before else None
        t0 = time.perf_counter()
        r = fn(arg)
        out.append((time.perf_counter() - t0) * 1e3)
        if after:
            after(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from getdist_amd._lib import Context
    from getdist_amd.mcsamples import MCSamples

    samples = np.random.default_rng(20261019).random((a.cols, a.rows)).T  # (rows, cols), column-major
    print("samples: %d x %d, %.2f GB" % (a.rows, a.cols, samples.nbytes / 1e9), flush=True)
    s = MCSamples(samples=samples, names=["p%d" % j for j in range(a.cols)])
    print("resident", flush=True)

    def fresh():
        return Context(0)

    def closed(ctx):
        ctx.close()

    def clone(ctx):
        ctx.clone_samples(s.ctx)  # (allocates, copies, returns when the copies are complete)
        return ctx

    def upload(ctx):
        ctx.upload(samples)
        return ctx

    def copy(_):
        return s.copy()

    def check_and_close(c):
        assert c.ctx is not s.ctx and np.array_equal(c.means, s.means)
        c.ctx.close()

    closed(clone(fresh())), closed(upload(fresh()))  # warm-up: allocator, first use of the copy paths
    t_clone = timed(clone, a.calls, fresh, closed)
    print("clone done", flush=True)
    t_upload = timed(upload, a.calls, fresh, closed)
    print("upload done", flush=True)
    t_copy = timed(copy, a.calls, None, check_and_close)
    t_host = timed(lambda _: samples.copy(order="K"), a.calls)  # what the host mirror of the copy costs by itself
    c = s.copy()
    same = bool(np.max(np.abs(c.ctx.cov()[1] - s.ctx.cov()[1])) <= 1e-12 * np.max(np.abs(s.fullcov)))
    res = dict(rows=a.rows, cols=a.cols, bytes=int(samples.nbytes), weights="unit", calls=a.calls,
               copy_ms=t_copy, copy_ms_median=float(np.median(t_copy)),
               clone_ms=t_clone, clone_ms_median=float(np.median(t_clone)),
               clone_GBps=float(2 * samples.nbytes / 1e6 / np.median(t_clone)),  # read + write
               upload_ms=t_upload, upload_ms_median=float(np.median(t_upload)),
               upload_GBps=float(samples.nbytes / 1e6 / np.median(t_upload)),
               host_array_copy_ms=t_host, host_array_copy_ms_median=float(np.median(t_host)),
               copy_statistics_match=same)
    print("copy() %.1f ms, of which gd_clone_samples %.1f ms (%.0f GB/s read + write) and the host array's copy %.1f ms; "
          "upload of the same array %.1f ms (%.1f GB/s); medians of %d calls"
          % (res["copy_ms_median"], res["clone_ms_median"], res["clone_GBps"], res["host_array_copy_ms_median"],
             res["upload_ms_median"], res["upload_GBps"], a.calls))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python scripts/bench_copy.py", result=res), f, indent=1)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
