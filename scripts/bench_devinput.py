"""Times the ways a sample set of 1e7 x 50 values reaches the device, in one process on one machine; no threshold but one:
the fp64 row-major gd_upload_device call must beat gd_upload of the same array from page-locked host memory.

    python scripts/bench_devinput.py [--rows 10000000] [--cols 50] [--calls 5] [--out profiles/devinput_throughput.json]

Measured (one warm-up call each, then ``--calls`` timed calls, medians reported, every call into a fresh context and timed
from the host until the call has returned, which is when the copy is complete):
  * Context.upload_device (gd_upload_device) from device memory: fp64 row-major, fp32 row-major, fp64 column-major;
  * Context.upload (gd_upload) of the same fp64 row-major values from page-locked host memory;
  * gd_memcpy_d2d of the same number of bytes (4 GB read + 4 GB written), the device-copy rate the first is stated against;
  * the MCSamples constructor end to end from a torch tensor on the GPU, and the way a user had to go before:
    ``MCSamples(samples=x.cpu().numpy())`` (torch is imported before the library is loaded: after it, torch sees no GPU;
    without torch the same from a device block and its pageable download).  ``--no-constructor`` leaves this part out."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, calls, before=None, after=None):
    """Milliseconds of ``fn(before())`` per call, after one warm-up call; ``after(result)`` cleans up outside the timed region."""
    out = []
    for k in range(calls + 1):
        arg = before() if before else None
        t0 = time.perf_counter()
        r = fn(arg)
        ms = (time.perf_counter() - t0) * 1e3
        if k:
            out.append(ms)
        if after:
            after(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=50)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-constructor", action="store_true", help="the native calls only (for a kernel trace)")
    a = ap.parse_args()
    torch = None
    if not a.no_constructor:
        try:  # before libgdhip.so is loaded: imported after it, torch reports no GPU
            import torch
        except ImportError:
            pass
    from getdist_amd import devarray
    from getdist_amd._lib import Context
    from getdist_amd.mcsamples import MCSamples

    feeder = Context(0)
    host = feeder.pinned_block((a.rows, a.cols))  # page-locked, row-major
    rng = np.random.default_rng(20261020)
    for r0 in range(0, a.rows, 1 << 20):
        host[r0:r0 + (1 << 20)] = rng.random(host[r0:r0 + (1 << 20)].shape, dtype=np.float32)  # (exact in fp32 as well)
    nbytes = host.nbytes
    print("samples: %d x %d, %.2f GB" % (a.rows, a.cols, nbytes / 1e9), flush=True)

    def on_device(arr, shape, strides, dtype):
        buf = feeder.alloc(arr.nbytes)
        buf.from_host(arr)
        return devarray.DevArray(buf.ptr, shape, strides, dtype, owner=buf)

    row64 = on_device(host, (a.rows, a.cols), (a.cols, 1), devarray.GD_DT_F64)
    bcol = feeder.alloc(nbytes)
    col64 = devarray.DevArray(bcol.ptr, (a.rows, a.cols), (1, a.rows), devarray.GD_DT_F64, owner=bcol)
    spare = feeder.alloc(nbytes)
    row32 = None
    for r0 in range(0, a.rows, 1 << 20):  # fp32 copy and column-major copy, block by block (no second 4-GB host array)
        blk = host[r0:r0 + (1 << 20)]
        if row32 is None:
            b32 = feeder.alloc(a.rows * a.cols * 4)
            row32 = devarray.DevArray(b32.ptr, (a.rows, a.cols), (a.cols, 1), devarray.GD_DT_F32, owner=b32)
        blk32 = blk.astype(np.float32)  # (held in a name: the copy reads it through a raw pointer)
        feeder._check(feeder.lib.gd_memcpy_h2d(feeder.h, row32.ptr + r0 * a.cols * 4, blk32.ctypes.data, blk32.nbytes))
    fill = Context(0)
    assert fill.upload_device([row64])  # the column-major source: the resident columns of an upload, copied out
    for j in range(a.cols):
        feeder._check(feeder.lib.gd_memcpy_d2d(feeder.h, col64.ptr + j * a.rows * 8, fill.column_ptr(j), a.rows * 8))
    feeder.sync()
    check = fill.cov()[1]
    fill.close()
    print("sources resident", flush=True)

    def fresh():
        return Context(0)

    def closed(ctx):
        ctx.close()

    def from_device(desc):
        def go(ctx):
            assert ctx.upload_device([desc])
            return ctx
        return go

    def from_pinned(ctx):
        ctx.upload(host)
        return ctx

    def d2d(_):
        feeder.lib.gd_memcpy_d2d(feeder.h, spare.ptr, row64.ptr, nbytes)
        feeder.sync()

    res = dict(rows=a.rows, cols=a.cols, bytes=int(nbytes), calls=a.calls)
    for key, fn in (("device_f64_row_major", from_device(row64)), ("device_f32_row_major", from_device(row32)),
                    ("device_f64_column_major", from_device(col64)), ("pinned_host_f64_row_major", from_pinned)):
        t = timed(fn, a.calls, fresh, closed)
        res[key + "_ms"], res[key + "_ms_median"] = t, float(np.median(t))
        print("%s: %.2f ms" % (key, res[key + "_ms_median"]), flush=True)
    t = timed(d2d, a.calls)
    res["memcpy_d2d_ms"], res["memcpy_d2d_ms_median"] = t, float(np.median(t))
    res["device_f64_row_major_GBps"] = float(2 * nbytes / 1e6 / res["device_f64_row_major_ms_median"])  # read + write
    res["memcpy_d2d_GBps"] = float(2 * nbytes / 1e6 / res["memcpy_d2d_ms_median"])
    res["device_f64_row_major_fraction_of_d2d_rate"] = res["memcpy_d2d_ms_median"] / res["device_f64_row_major_ms_median"]
    c = fresh()
    assert c.upload_device([row64])
    res["statistics_match"] = bool(np.array_equal(c.cov()[1], check))
    c.close()

    have_torch = torch is not None and torch.cuda.is_available()
    if not a.no_constructor:
        if have_torch:
            x = torch.rand(a.rows, a.cols, device="cuda", dtype=torch.float64)
            torch.cuda.synchronize()
            source, to_host = "torch.Tensor", (lambda: x.cpu().numpy())
        else:  # the same two ways without torch: the device block above, and its pageable download (what .cpu().numpy() is)
            x, source, to_host = row64, "device block (torch sees no GPU)", (lambda: row64.owner.to_host((a.rows, a.cols)))
        names = ["p%d" % j for j in range(a.cols)]
        calls = max(1, min(a.calls, 3))
        done = (lambda s: s.ctx.close())
        t_dev = timed(lambda _: MCSamples(samples=x, names=names), calls, None, done)
        t_host = timed(lambda _: MCSamples(samples=to_host(), names=names), calls, None, done)
        res.update(constructor_source=source, constructor_device_ms=t_dev, constructor_device_ms_median=float(np.median(t_dev)),
                   constructor_host_ms=t_host, constructor_host_ms_median=float(np.median(t_host)))
        print("constructor (%s): %.1f ms from the device array, %.1f ms through a host copy of it"
              % (source, res["constructor_device_ms_median"], res["constructor_host_ms_median"]), flush=True)
    print("gd_upload_device fp64 row-major %.2f ms (%.0f GB/s read + write, %.2f of the device-copy rate: gd_memcpy_d2d %.2f ms); "
          "fp32 %.2f ms; column-major %.2f ms; gd_upload from page-locked memory %.2f ms; medians of %d calls"
          % (res["device_f64_row_major_ms_median"], res["device_f64_row_major_GBps"],
             res["device_f64_row_major_fraction_of_d2d_rate"], res["memcpy_d2d_ms_median"], res["device_f32_row_major_ms_median"],
             res["device_f64_column_major_ms_median"], res["pinned_host_f64_row_major_ms_median"], a.calls))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python scripts/bench_devinput.py", result=res), f, indent=1)
    if not (res["statistics_match"] and res["device_f64_row_major_ms_median"] < res["pinned_host_f64_row_major_ms_median"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
