"""Times the ways the resident samples (1e7 x 50) leave the library as a device array, in one process on one machine.  No
threshold: the figures and their ratios are recorded.

    python scripts/bench_devexport.py [--rows 10000000] [--cols 50] [--calls 5] [--out profiles/devexport_throughput.json]

Measured (one warm-up call each, then ``--calls`` timed calls; median, minimum and maximum reported; every call is timed from
the host until it has returned, which -- with no consumer stream -- is when the destination is written):
  * Context.export_device (gd_export_device) into a destination allocated beforehand: all rows as fp64 and as fp32 row-major,
    fp64 column-major, 8 listed columns as fp32, a p = 0.5 and a p = 0.01 device mask (fp64 row-major), and half the rows as
    fp64 into a view whose strides force the 32 x 32 tile path (the stand-in for the 32 x 32 tile of gd_download_samples,
    whose kernel cannot be launched without its copy to the host);
  * getDeviceSamples end to end (allocation of the result included) for the same cases, and one with a derived expression;
  * gd_memcpy_d2d of the bytes the fp64 export reads plus writes (4 GB read + 4 GB written): the device-copy rate;
  * the route as it stood: gd_download_samples into page-locked memory plus gd_upload of the result into another context
    (the host's fancy indexing and dtype cast, which that route also pays, are not timed)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls):
    out = []
    for k in range(calls + 1):
        t0 = time.perf_counter()
        r = fn()
        ms = (time.perf_counter() - t0) * 1e3
        del r
        if k:
            out.append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from getdist_amd import devarray
    from getdist_amd._lib import Context
    from getdist_amd.mcsamples import MCSamples

    N, n = a.rows, a.cols
    feeder = Context(0)
    # the source: one block of 2^20 random rows repeated down the array (filled by copies of one page-locked block)
    blk_rows = min(N, 1 << 20)
    blk = feeder.pinned_block((blk_rows, n))
    blk[:] = np.random.default_rng(20261021).standard_normal((blk_rows, n))
    src = feeder.alloc(N * n * 8)
    for r0 in range(0, N, blk_rows):
        rows = min(blk_rows, N - r0)
        feeder._check(feeder.lib.gd_memcpy_h2d(feeder.h, src.ptr + r0 * n * 8, blk.ctypes.data, rows * n * 8))
    names = ["p%d" % j for j in range(n)]
    mc = MCSamples(samples=devarray.DevArray(src.ptr, (N, n), (n, 1), devarray.GD_DT_F64, owner=src), names=names)
    ctx = mc.ctx
    src.free()
    nbytes = N * n * 8
    print("resident: %d x %d, %.2f GB" % (N, n, nbytes / 1e9), flush=True)

    dst = feeder.alloc(nbytes)
    rng = np.random.default_rng(7)
    masks = {}
    for key, prob in (("mask_p50", 0.5), ("mask_p01", 0.01)):
        m = rng.random(N) < prob
        buf = feeder.alloc(N)
        buf.from_host(m.view(np.uint8))
        masks[key] = (buf, m, int(m.sum()))
    eight = list(range(0, n, max(n // 8, 1)))[:8]
    every = list(range(n))

    def view(rows, cols, rs, cs, code):
        return devarray.DevArray(dst.ptr, (rows, cols), (rs, cs), code, owner=dst)

    F64, F32 = devarray.GD_DT_F64, devarray.GD_DT_F32
    native = {
        "all_f64_row_major": (None, every, view(N, n, n, 1, F64)),
        "all_f32_row_major": (None, every, view(N, n, n, 1, F32)),
        "all_f64_column_major": (None, every, view(N, n, 1, N, F64)),
        "cols8_f32_row_major": (None, eight, view(N, len(eight), len(eight), 1, F32)),
        "mask_p50_f64_row_major": (("mask", masks["mask_p50"][0]), every, view(masks["mask_p50"][2], n, n, 1, F64)),
        "mask_p01_f64_row_major": (("mask", masks["mask_p01"][0]), every, view(masks["mask_p01"][2], n, n, 1, F64)),
        "half_f64_tile_path": (("range", 0, N // 2), every, view(N // 2, n, 2 * n, 2, F64)),  # every other element of the block
    }
    res = dict(rows=N, cols=n, bytes=int(nbytes), calls=a.calls, native={}, end_to_end={})

    def record(group, key, t, moved):
        res[group][key] = dict(ms=t, ms_median=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)),
                               GBps=float(moved / 1e6 / np.median(t)))
        print("%s %s: %.2f ms (%.2f .. %.2f), %.0f GB/s read + write" % (group, key, np.median(t), min(t), max(t), res[group][key]["GBps"]),
              flush=True)

    for key, (rows, cols, dest) in native.items():
        moved = dest.shape[0] * dest.shape[1] * (8 + dest.itemsize)
        record("native", key, timed(lambda: ctx.export_device(rows=rows, cols=cols, dest=dest), a.calls), moved)

    p = mc.getDeviceParams()
    e2e = {
        "all_f64_row_major": dict(),
        "all_f32_row_major": dict(dtype=np.float32),
        "all_f64_column_major": dict(order="F"),
        "cols8_f32_row_major": dict(params=[names[j] for j in eight], dtype=np.float32),
        "mask_p50_f64_row_major": dict(rows=masks["mask_p50"][1]),
        "mask_p01_f64_row_major": dict(rows=masks["mask_p01"][1]),
        "expr_mask_f64_row_major": dict(rows=p.p0 > 0.0),
        "cols8_and_derived_f32": dict(params=[names[j] for j in eight] + [p.p0 * np.sqrt(np.abs(p.p1) / 0.3)], dtype=np.float32),
    }
    dst.free()
    feeder.release_cached_blocks()  # (the results of getDeviceSamples are allocations of their own)
    for key, kw in e2e.items():
        t, shape = [], None
        for k in range(a.calls + 1):
            t0 = time.perf_counter()
            out = mc.getDeviceSamples(**kw)
            ms = (time.perf_counter() - t0) * 1e3
            shape, size = out.shape, out.itemsize
            del out
            if k:
                t.append(ms)
        record("end_to_end", key, t, shape[0] * shape[1] * (8 + size))

    a_buf, b_buf = feeder.alloc(nbytes), feeder.alloc(nbytes)

    def d2d():
        feeder.lib.gd_memcpy_d2d(feeder.h, b_buf.ptr, a_buf.ptr, nbytes)
        feeder.sync()

    t = timed(d2d, a.calls)
    res["memcpy_d2d"] = dict(ms=t, ms_median=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)),
                             GBps=float(2 * nbytes / 1e6 / np.median(t)))
    a_buf.free(), b_buf.free()
    feeder.release_cached_blocks()
    other = Context(0)

    def round_trip():
        host = ctx.download_samples()
        other.upload(host)

    t = timed(round_trip, max(1, min(a.calls, 2)))
    res["download_plus_upload"] = dict(ms=t, ms_median=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)))
    other.close()
    d2d_ms = res["memcpy_d2d"]["ms_median"]
    res["ratios"] = {
        "all_f64_row_major_fraction_of_d2d_rate": d2d_ms / res["native"]["all_f64_row_major"]["ms_median"],
        "all_f64_column_major_fraction_of_d2d_rate": d2d_ms / res["native"]["all_f64_column_major"]["ms_median"],
        "slab_path_rate_over_tile_path_rate": res["native"]["all_f64_row_major"]["GBps"] / res["native"]["half_f64_tile_path"]["GBps"],
        "download_plus_upload_over_getDeviceSamples": res["download_plus_upload"]["ms_median"] / res["end_to_end"]["all_f64_row_major"]["ms_median"],
    }
    print("memcpy_d2d %.2f ms; download + upload %.1f ms; ratios %s" % (d2d_ms, res["download_plus_upload"]["ms_median"],
                                                                         json.dumps(res["ratios"])), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python scripts/bench_devexport.py", result=res), f, indent=1)
    mc.ctx.close()
    feeder.close()


if __name__ == "__main__":
    main()
