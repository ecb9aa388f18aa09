"""Dump what every entry point of csrc/stats.hip returns, on fixed seeded inputs, into one .npz: run it with two builds of
the library and compare the files array by array (np.array_equal) to show that a change of the host code kept every route
bit for bit.  The inputs are those of tests/test_gpu_stats_routes.py (every covariance route, the single-lag kernel, the
2D lag sums) and the `data` fixture of tests/test_gpu_primitives.py (300 001 rows x 10 columns, weighted and not).

    python scripts/stats_dump.py --out stats.npz            # then: --compare a.npz b.npz
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COV_WIDTHS = [1, 31, 32, 47, 63, 79, 95, 111, 143, 191, 207, 208, 209]


def content_hash(arrays):
    """sha256 over names, types, shapes and bytes of the arrays (an .npz file's own bytes carry time stamps)"""
    h = hashlib.sha256()
    for k in sorted(arrays.keys()):
        a = np.ascontiguousarray(arrays[k])
        h.update(("%s %s %s\n" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def dump(out):
    from getdist_amd import synth
    from getdist_amd._lib import Context

    ctx = Context(0)
    res = {}

    def put(name, value):
        assert name not in res, name
        res[name] = np.array(value)

    # ---- the shapes of tests/test_gpu_stats_routes.py
    r = np.random.default_rng(2024)
    N, ncols, lo, hi = 3001, 230, 1, 3000
    s = r.standard_normal((N, ncols)) * r.uniform(0.5, 2.0, ncols) + r.uniform(-5.0, 5.0, ncols)
    for wname, w in (("unit", None), ("real", r.random(N) + 0.25)):
        ctx.upload(s, w)
        for twopass in (False, True):
            if twopass:
                os.environ["GDHIP_COV_TWOPASS"] = "1"
            try:
                for m in COV_WIDTHS:
                    cols = np.random.default_rng(m).permutation(ncols)[:m]
                    means, cov, norm, mm = ctx.cov(cols=cols, lo=lo, hi=hi, minmax=True)
                    tag = "cov_%s_%s_m%d" % (wname, "twopass" if twopass else "default", m)
                    put(tag + "_means", means), put(tag + "_cov", cov), put(tag + "_norm", norm), put(tag + "_minmax", mm)
            finally:
                os.environ.pop("GDHIP_COV_TWOPASS", None)
    r = np.random.default_rng(77)
    N = 5001
    x = np.cumsum(r.standard_normal((N, 2)), axis=0) * 0.05 + r.standard_normal((N, 2))
    c = np.array([1.0 / (4 * 0.3**2), 0.8])
    for wname, w in (("unit", None), ("real", r.random(N) + 0.25)):
        ctx.upload(x, w)
        put("lag9_" + wname, ctx.kde_lag_sums_batch([0, 1], c, [1, 2, 3, 7, 50, 1000, N // 2, N // 2 + 4, N - 2]))
        put("lag2d_" + wname, ctx.kde_lag_sums_2d(1, 0, [2.5, -1.2, 1.75], [1, 2, 7, N // 2, N // 2 + 4]))
        for lags in ([N // 2 + d for d in range(5)] + [1, 2], [N // 2 + d for d in range(5)] + [1], [1, 2, 7]):
            put("lag_multi_%s_%d" % (wname, len(lags)), ctx.kde_lag_sums_batch([0, 1], c, lags))
        os.environ["GDHIP_KDE_LAG_UNFOLDED"] = "1"
        try:
            put("lag_unfolded_" + wname, ctx.kde_lag_sums_batch([0, 1], c, [N // 2 + d for d in range(5)] + [1, 2]))
        finally:
            del os.environ["GDHIP_KDE_LAG_UNFOLDED"]

    # ---- the `data` fixture of tests/test_gpu_primitives.py
    N = 300_001
    fracs = np.array([0.001, 0.999] + list(np.linspace(0.1, 0.9, 9)) + [1.0, 2.0, 0.0])
    for wname in ("weighted", "unit"):
        s, w, _, _ = synth.block_recipe(10, N, weighted=(wname == "weighted"), stream=21)
        ctx.upload(s, w)
        norm = N if w is None else w.sum()
        st = ctx.col_stats()
        put("col_stats_" + wname, st)
        put("col_stats_range_" + wname, ctx.col_stats(lo=1001, hi=200_000))
        ws = ctx.weight_stats(thresh=2.0)
        put("weight_stats_" + wname, [ws["norm"], ws["max_w"], ws["sum_w2"], ws["n_above"]])
        for tag, kw in (("all", {}), ("sub", dict(cols=[3, 7, 1], lo=1001, hi=200_000))):
            means, cov, nrm, mm = ctx.cov(minmax=True, **kw)
            put("cov_%s_%s" % (tag, wname), np.concatenate([means, cov.ravel(), [nrm], mm.ravel()]))
        put("col_minmax_" + wname, ctx.col_minmax([0, 4, 9], lo=5, hi=N - 3))
        put("col_minmax_cond_" + wname, ctx.col_minmax([0, 4, 9], cond_col=2, cond_below=float(st[2, 2])))
        cols = [0, 4, 9]
        targets = np.tile(norm * fracs[:11], (len(cols), 1))
        mm = st[cols, :2]
        put("quantiles_radix_" + wname, ctx.quantiles(cols, targets))
        put("quantiles_radix_range_" + wname, ctx.quantiles(cols, targets * 0.5, lo=1001, hi=200_000))
        put("quantiles_linear_" + wname, ctx.quantiles(cols, targets, minmax=mm))
        put("quantiles_linear_range_" + wname, ctx.quantiles(cols, targets * 0.5, lo=1001, hi=200_000, minmax=mm))
        q, probe = ctx.quantiles_probe(cols, targets, mm, st[cols, 2])
        put("quantiles_probe_q_" + wname, q)
        put("quantiles_probe_lags_" + wname, np.zeros(0) if probe is None else probe)
        os.environ["GDHIP_QLIN_UNFUSED"] = "1"
        try:
            q, probe = ctx.quantiles_probe(cols, targets, mm, st[cols, 2])
            put("quantiles_unfused_q_" + wname, q)
            put("quantiles_unfused_probe_done_" + wname, probe is not None)
        finally:
            del os.environ["GDHIP_QLIN_UNFUSED"]
        put("autocov_40_" + wname, ctx.autocov_lags(2, st[2, 2], 0, 40))
        put("autocov_5_" + wname, ctx.autocov_lags(2, st[2, 2], 37, 5))
        put("autocov_range_" + wname, ctx.autocov_lags_range_batch([1, 2, 8], st[[1, 2, 8], 2], 1001, 200_000, 0, 12))
        put("kde_lag_" + wname, ctx.kde_lag_sums(2, 1.0 / (4 * 0.3**2), [1, 2, 7, N // 2, N // 2 + 4]))
        put("kde_lag_neff_" + wname, ctx.kde_lag_sums_batch([0, 2, 5], [2.0, 2.7, 0.9], [N // 2 + d for d in range(5)] + [1, 2]))
    # tied values: the linear route's lists overflow and the radix passes finish the call
    r = np.random.default_rng(5)
    t = np.round(r.standard_normal((200_000, 2)) * 3.0)
    ctx.upload(t, None)
    tg = np.tile(200_000 * fracs[:11], (2, 1))
    put("quantiles_tied", ctx.quantiles([0, 1], tg, minmax=np.stack([t.min(axis=0), t.max(axis=0)], axis=1)))
    ctx.close()
    np.savez(out, **res)
    print("wrote %s: %d arrays, content sha256 %s" % (out, len(res), content_hash(res)))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    equal = {k: bool(k in B.files and np.array_equal(A[k], B[k], equal_nan=True)) for k in A.files}
    for k in B.files:
        equal.setdefault(k, False)
    print(json.dumps({"arrays": len(equal), "all_equal": all(equal.values()), "differ": [k for k, v in equal.items() if not v],
                      "content_sha256": [content_hash(A), content_hash(B)]}))
    return 0 if all(equal.values()) else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    dump(args.out or "stats_dump.npz")
