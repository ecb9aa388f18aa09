"""Times the weight-one draw at N = 1e7 rows: the device call up to "indices on the host" (gd_draw_single_rows with the
PCG64 regenerated per thread, plus the D2H of the kept rows) next to the numpy expression of the reference on the same
machine's CPU, and checks that the two lists are equal.

    python scripts/bench_single_draw.py [--rows 10000000] [--calls 20] [--warmup 3] [--thin 0] [--out FILE]

--thin 0 takes the default of makeSingleSamples (about max_scatter_points = 2000 rows kept); the second line printed is
thin = 1 (about norm / max weight rows kept), where the D2H of the list is the larger share."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(ctx, w, mx, thin, seed, calls, warmup):
    N = len(w)
    s = np.random.default_rng(seed).bit_generator.state["state"]
    pcg = (s["state"], s["inc"])

    def device():
        buf, K = ctx.draw_single_rows(mx, thin, 0, pcg=pcg)
        out = buf.to_host((K,), dtype=np.int32).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
        buf.free()
        return out

    def host():
        return np.nonzero(np.random.default_rng(seed).random(N) <= w / (mx * thin))[0]

    for _ in range(warmup):
        got = device()
    t_dev, t_np = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        got = device()  # (the entry blocks until the list is complete; to_host blocks until it is on the host)
        t_dev.append((time.perf_counter() - t0) * 1e3)
    for _ in range(max(3, calls // 4)):
        t0 = time.perf_counter()
        want = host()
        t_np.append((time.perf_counter() - t0) * 1e3)
    t_dev, t_np = np.array(t_dev), np.array(t_np)
    return dict(rows=N, thin=float(thin), kept=int(len(want)), equal=bool(np.array_equal(got, want)),
                device_ms_median=float(np.median(t_dev)), device_ms_min=float(t_dev.min()), device_ms_max=float(t_dev.max()),
                numpy_ms_median=float(np.median(t_np)), numpy_ms_min=float(t_np.min()),
                weight_bytes_read=2 * 8 * N, calls=calls, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--thin", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from getdist_amd._lib import Context

    r = np.random.default_rng(1)
    w = r.integers(1, 30, a.rows).astype(float)
    mx = float(np.max(w))
    ctx = Context(0)
    ctx.upload(np.zeros((a.rows, 1)), w)
    thin = a.thin or max(1.0, float(np.sum(w)) / mx / 2000)
    results = [measure(ctx, w, mx, t, 12345, a.calls, a.warmup) for t in (thin, 1.0)]
    ctx.close()
    for res in results:
        print("draw N=%d thin=%.4g kept=%d equal=%s: device (call + D2H of the rows) median %.3f ms (min %.3f, max %.3f) over "
              "%d calls after %d warm-ups; numpy random + compare + nonzero median %.1f ms (min %.1f)"
              % (res["rows"], res["thin"], res["kept"], res["equal"], res["device_ms_median"], res["device_ms_min"],
                 res["device_ms_max"], res["calls"], res["warmup"], res["numpy_ms_median"], res["numpy_ms_min"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python scripts/bench_single_draw.py", results=results), f, indent=1)
    if not all(res["equal"] for res in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
