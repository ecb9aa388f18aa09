"""
MCSamples.PCA on the device (gd_pca_corr + gd_pca_project): prints ONE JSON line.

  c3   N rows x 50 parameters of the C3 recipe, all of them, default maps
  c5   2e6 rows x 200 parameters of the block recipe (the C5 width), default maps

Per shape: device time of each entry (wall time of the native call, which blocks until its results are on the host),
end-to-end PCA() time (median and min after warm-up), bytes and flops per pass, and the achieved fraction of the HBM
(8 TB/s) and fp64 (78.6 TFLOP/s, matrix or vector) roofs.

    python scripts/bench_pca.py [--rows N] [--c5-rows N] [--steps K] [--warmup W]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from getdist_amd import synth  # noqa: E402
from getdist_amd.mcsamples import MCSamples  # noqa: E402

HBM_BPS, FP64_FLOPS = 8.0e12, 78.6e12


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def model(N, n, nall, weighted):
    """bytes read and fp64 flops of the four passes (columns once per pass; weights once; products: 2 flops each)"""
    wb = 8 * N if weighted else 0
    ceil16 = lambda k: (k + 15) // 16 * 16  # noqa: E731
    proj = 2.0 * N * n * n  # U z per row (each projection pass)
    passes = {
        "corr_sums": dict(bytes=8 * N * n + wb, flops=2.0 * N * ceil16(n + 1) * 16),
        "corr_cross": dict(bytes=8 * N * n + wb, flops=2.0 * N * ceil16(n) * ceil16(n) / 2),
        "proj_sums": dict(bytes=8 * N * n + wb, flops=proj + 2.0 * N * ceil16(n + 1) * 16),
        "proj_cross": dict(bytes=8 * N * (n + nall) + wb, flops=proj + 2.0 * N * ceil16(n) * (ceil16(n) / 2 + ceil16(nall))),
    }
    return passes


def run(name, s, w, names, steps, warmup):
    mc = MCSamples(samples=s, weights=w, names=names)
    N, n = s.shape
    ctx = mc.ctx
    dev = {"corr": [], "project": []}
    orig_c, orig_p = ctx.pca_corr, ctx.pca_project

    def corr(*a, **k):
        t0 = time.perf_counter()
        r = orig_c(*a, **k)
        dev["corr"].append(time.perf_counter() - t0)
        return r

    def project(*a, **k):
        t0 = time.perf_counter()
        r = orig_p(*a, **k)
        dev["project"].append(time.perf_counter() - t0)
        return r

    ctx.pca_corr, ctx.pca_project = corr, project
    med, mn = timed(lambda: mc.PCA(names), steps, warmup)
    tc, tp = float(np.median(dev["corr"][warmup:])), float(np.median(dev["project"][warmup:]))
    passes = model(N, n, n, w is not None)
    bc = passes["corr_sums"]["bytes"] + passes["corr_cross"]["bytes"]
    fc = passes["corr_sums"]["flops"] + passes["corr_cross"]["flops"]
    bp = passes["proj_sums"]["bytes"] + passes["proj_cross"]["bytes"]
    fp = passes["proj_sums"]["flops"] + passes["proj_cross"]["flops"]
    return dict(shape=name, rows=N, params=n, weighted=w is not None,
                pca_corr_s=tc, pca_project_s=tp, pca_e2e_median_s=med, pca_e2e_min_s=mn,
                passes=passes,
                corr_hbm_frac=bc / tc / HBM_BPS, corr_fp64_frac=fc / tc / FP64_FLOPS,
                project_hbm_frac=bp / tp / HBM_BPS, project_fp64_frac=fp / tp / FP64_FLOPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--c5-rows", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    s, w, names, _ = synth.config_c3(a.rows, 50)
    c3 = run("c3", s, w, names, a.steps, a.warmup)
    del s, w
    s, w, names, _ = synth.block_recipe(200, a.c5_rows, weighted=True, stream=5)
    c5 = run("c5_width", s, w, names, max(1, a.steps // 2), a.warmup)
    print(json.dumps(dict(metric="pca", c3=c3, c5_width=c5)))


if __name__ == "__main__":
    main()
