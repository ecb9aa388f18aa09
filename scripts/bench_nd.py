"""
Raw N-D densities on the device (gd_histnd_batch): prints ONE JSON line.

  single   one 3-parameter getRawNDDensityGridData with meanlikes + maxlikes over the C3 columns (N rows resident)
  batch    all C(n, 3) 3D raw densities of the C3 parameters (getRawNDDensities, get_density=True) in batched calls

    python scripts/bench_nd.py [--rows N] [--params n] [--steps K] [--warmup W]
"""

import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from getdist_amd import synth  # noqa: E402
from getdist_amd.mcsamples import MCSamples  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--params", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    s, w, names, ranges = synth.config_c3(a.rows, a.params)
    z = (s[:, :3] - s[:, :3].mean(axis=0)) / s[:, :3].std(axis=0)
    loglikes = 0.5 * np.sum(z * z, axis=1) + 11.0
    del z
    mc = MCSamples(samples=s, weights=w, loglikes=loglikes, names=names, ranges=ranges)
    trio = names[5:8]
    mc.getLikeStats()
    single_med, single_min = timed(lambda: mc.getRawNDDensityGridData(trio, meanlikes=True, maxlikes=True), a.steps, a.warmup)
    triples = [list(t) for t in itertools.combinations(range(a.params), 3)]
    ctx = mc.ctx
    calls0, native_s = [0], [0.0]
    orig = ctx.histnd_batch

    def counting(*args, **kw):  # native calls and their wall time (index columns, kernels, copies of the grids)
        calls0[0] += 1
        t0 = time.perf_counter()
        r = orig(*args, **kw)
        native_s[0] += time.perf_counter() - t0
        return r

    ctx.histnd_batch = counting
    bsteps = max(1, a.steps // 2)
    batch_med, batch_min = timed(lambda: mc.getRawNDDensities(triples, get_density=True), bsteps, a.warmup)
    calls = calls0[0] // (a.warmup + bsteps)
    native = native_s[0] / (a.warmup + bsteps)
    adds = float(len(triples)) * a.rows
    print(json.dumps(dict(
        metric="raw_nd_densities", rows=a.rows, params=a.params,
        single_3d_meanlikes_maxlikes_s=single_med, single_3d_min_s=single_min,
        batch_densities=len(triples), batch_native_calls=calls, batch_s=batch_med, batch_min_s=batch_min, batch_native_s=native,
        batch_densities_per_s=len(triples) / batch_med, batch_native_adds_per_s=adds / native)))


if __name__ == "__main__":
    main()
