"""
Throughput of the chain ingestion on one GPU: a chain file the export wrote (N rows x (50 parameters + weight + loglike)
as "%.8e" text, on tmpfs) read back by chainfiles.loadNumpyTxt.

Per N it reports, from the same process:
  scan_ms          gd_parse_scan of the whole text, resident on the device, between device events
  parse_rows_ms    gd_parse_rows of the same text (its own scan pass included), between device events
  h2d_ms / d2h_ms  the copy of the text from page-locked memory to the device / of the parsed block back (host clock)
  device_s         loadNumpyTxt(path, ctx=ctx) end to end: file read, copies, kernels, fix-up
  fixes            tokens the device left to the host's float()
  host_s, loadtxt_s  the host route of loadNumpyTxt without a context (pandas round_trip when installed, else np.loadtxt)
                   and np.loadtxt itself on the same file and machine
Medians of --repeats runs after one warm-up; the host routes run once (--host-rows caps their file).  One JSON line on
stdout; --out also writes it to a file.

    python scripts/bench_ingest.py --rows 200000 2000000 --out profiles/ingest_throughput.json
"""

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from getdist_amd import chainfiles  # noqa: E402
from getdist_amd._lib import GD_FMT_SRC_WEIGHT, Context  # noqa: E402

NPAR = 50


def median(xs):
    return float(np.median(xs))


def write_chain(ctx, N, path):
    rng = np.random.default_rng(1)
    s = np.empty((N, NPAR), order="F")
    for j in range(NPAR):
        s[:, j] = rng.standard_normal(N) * 10.0 ** (j % 7 - 3)
    ctx.upload(s, rng.integers(1, 20, N).astype(np.float64))
    srcs = [GD_FMT_SRC_WEIGHT, ctx.set_extra_column(ctx.EXTRA_COLS - 1, rng.uniform(0, 40, N))] + list(range(NPAR))
    chainfiles.write_text_rows(path, ctx, srcs, (0, N))


def bench(N, repeats, tmpfs, host_rows):
    ctx = Context(0)
    path = os.path.join(tmpfs, "bench_ingest_%d.txt" % os.getpid())
    small = path + ".host"
    try:
        write_chain(ctx, N, path)
        size = os.path.getsize(path)
        res = dict(rows=N, fields=NPAR + 2, text_bytes=size)

        host = ctx.pinned_array((size,), np.uint8)
        with open(path, "rb") as f:
            assert f.readinto(memoryview(host)) == size
        text = ctx.alloc(size)
        scan, parse, h2d, d2h = [], [], [], []
        out = None
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            ctx._check(ctx.lib.gd_memcpy_h2d(ctx.h, text.ptr, host.ctypes.data, size))
            c = (time.perf_counter() - t0) * 1e3
            ctx.timer_start()
            rc, rows, m, used = ctx.parse_scan(text, size, last=True)
            k1 = ctx.timer_stop_ms()
            assert (rc, rows, m, used) == (0, N, NPAR + 2, size)
            out = out or ctx.alloc(8 * m * rows)
            ctx.timer_start()
            rc, fixes, count = ctx.parse_rows(text, size, rows, m, out, rows)
            k2 = ctx.timer_stop_ms()
            assert rc == 0
            back = ctx.pinned_array((m * rows,), np.float64)
            t0 = time.perf_counter()
            ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, back.ctypes.data, out.ptr, back.nbytes))
            d = (time.perf_counter() - t0) * 1e3
            del back
            if it:
                scan.append(k1), parse.append(k2), h2d.append(c), d2h.append(d)
        text.free()
        out.free()
        del host
        res.update(scan_ms=median(scan), parse_rows_ms=median(parse), h2d_ms=median(h2d), d2h_ms=median(d2h), fixes=int(count),
                   scan_text_GBps=size / median(scan) / 1e6, parse_rows_text_GBps=size / median(parse) / 1e6,
                   h2d_GBps=size / median(h2d) / 1e6, d2h_GBps=8 * m * rows / median(d2h) / 1e6)

        times = []
        for it in range(repeats + 1):
            t0 = time.perf_counter()
            got = chainfiles.loadNumpyTxt(path, ctx=ctx)
            if it:
                times.append(time.perf_counter() - t0)
        assert got.shape == (N, NPAR + 2)
        res.update(device_s=median(times), device_text_GBps=size / median(times) / 1e9)

        k = min(host_rows, N)
        with open(path, "rb") as f, open(small, "wb") as g:  # the first k rows: the host routes are timed on them
            for _ in range(k):
                g.write(f.readline())
        t0 = time.perf_counter()
        ref = np.loadtxt(small)
        t_loadtxt = time.perf_counter() - t0
        t0 = time.perf_counter()
        hosted = chainfiles.loadNumpyTxt(small)
        t_host = time.perf_counter() - t0
        assert np.array_equal(got[:k].view(np.uint64), ref.view(np.uint64)), "device values differ from np.loadtxt"
        assert np.array_equal(hosted.view(np.uint64), ref.view(np.uint64))
        try:
            import pandas  # noqa: F401

            host_parser = "pandas round_trip"
        except ImportError:
            host_parser = "np.loadtxt"
        res.update(host_rows=k, host_parser=host_parser, host_slice_s=t_host, loadtxt_slice_s=t_loadtxt, host_s=t_host * N / k,
                   loadtxt_s=t_loadtxt * N / k, kernel_share_of_device_s=(median(scan) + median(parse)) / 1e3 / median(times))
        return res
    finally:
        for f in (path, small):
            if os.path.exists(f):
                os.remove(f)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[200_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=200_000)
    ap.add_argument("--tmpfs", default="/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(bench="ingest_throughput", format="%.8e", numpy=np.__version__,
               results=[bench(N, a.repeats, a.tmpfs, a.host_rows) for N in a.rows])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
