"""
Throughput of the chain export on one GPU: N rows x (50 parameters + weight + loglike) as "%.8e" text, columns resident.

Per N it reports, from the same process:
  kernel_ms_per_chunk   gd_format_rows of one chunk between device events (count pass + scan + write pass)
  d2h_ms_per_chunk      the copy of that chunk's text into page-locked memory (host clock around copy + synchronise)
  discard / tmpfs       write_text_rows end to end into a sink that drops the bytes / a file on tmpfs: seconds, text GB/s
  savetxt               np.savetxt of a 200 000-row slice of the same array on this host, scaled to N: the reference's cost
Medians of --repeats runs after one warm-up.  One JSON line on stdout; --out also writes it to a file.

    python scripts/bench_export.py --rows 1000000 10000000 --out profiles/export_throughput.json
"""

import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from getdist_amd import chainfiles  # noqa: E402
from getdist_amd._lib import GD_FMT_SRC_WEIGHT, Context, format_field_bytes  # noqa: E402

NPAR = 50
SLICE = 200_000


class Discard:
    def __init__(self):
        self.bytes = 0

    def write(self, data):
        self.bytes += len(data)


def median(xs):
    return float(np.median(xs))


def bench(N, repeats, tmpfs):
    rng = np.random.default_rng(1)
    s = np.empty((N, NPAR), order="F")
    for j in range(NPAR):  # the device layout, filled column by column
        s[:, j] = rng.standard_normal(N) * 10.0 ** (j % 7 - 3)
    w = rng.integers(1, 20, N).astype(np.float64)
    ll = rng.uniform(0, 40, N)
    ctx = Context(0)
    ctx.upload(s, w)
    srcs = [GD_FMT_SRC_WEIGHT, ctx.set_extra_column(ctx.EXTRA_COLS - 1, ll)] + list(range(NPAR))
    per_row = len(srcs) * format_field_bytes(0, 8)
    chunk = min(N, max(1, chainfiles.TEXT_CHUNK_BYTES // per_row))
    res = dict(rows=N, fields=len(srcs), chunk_rows=chunk)

    dev = ctx.alloc(chunk * per_row)
    host = ctx.pinned_array((chunk * per_row,), np.uint8)
    kms, cms = [], []
    for it in range(repeats + 1):
        ctx.timer_start()
        _, nbytes = ctx.format_rows(srcs, lo=0, hi=chunk, out=dev)
        k = ctx.timer_stop_ms()
        t0 = time.perf_counter()
        ctx.fetch_bytes_async(dev, host, nbytes)
        ctx.copy_sync()
        c = (time.perf_counter() - t0) * 1e3
        if it:
            kms.append(k), cms.append(c)
    dev.free()
    res.update(chunk_text_bytes=int(nbytes), kernel_ms_per_chunk=median(kms), d2h_ms_per_chunk=median(cms),
               kernel_text_GBps=nbytes / median(kms) / 1e6, d2h_GBps=nbytes / median(cms) / 1e6)
    del host

    sink = Discard()
    times = []
    for it in range(repeats + 1):
        sink.bytes = 0
        t0 = time.perf_counter()
        chainfiles.write_text_rows(sink, ctx, srcs, (0, N))
        if it:
            times.append(time.perf_counter() - t0)
    res.update(text_bytes=sink.bytes, discard_s=median(times), discard_text_GBps=sink.bytes / median(times) / 1e9)

    if tmpfs:
        path = os.path.join(tmpfs, "bench_export_%d.txt" % os.getpid())
        try:
            times = []
            for it in range(repeats + 1):
                t0 = time.perf_counter()
                chainfiles.write_text_rows(path, ctx, srcs, (0, N))
                if it:
                    times.append(time.perf_counter() - t0)
            assert os.path.getsize(path) == sink.bytes
            res.update(tmpfs_s=median(times), tmpfs_text_GBps=sink.bytes / median(times) / 1e9)
        except OSError as e:
            res["tmpfs_error"] = str(e)
        finally:
            for f in (path, path + ".tmp%d" % os.getpid()):
                if os.path.exists(f):
                    os.remove(f)

    k = min(SLICE, N)
    table = np.hstack((w[:k, None], ll[:k, None], s[:k]))
    t0 = time.perf_counter()
    ref = io.BytesIO()
    np.savetxt(ref, table, fmt="%.8e")
    t = time.perf_counter() - t0
    # the same rows from the device are the same bytes
    buf = io.BytesIO()
    chainfiles.write_text_rows(buf, ctx, srcs, (0, k))
    assert buf.getvalue() == ref.getvalue(), "device text differs from np.savetxt"
    res.update(savetxt_slice_rows=k, savetxt_slice_s=t, savetxt_scaled_s=t * N / k, speedup_discard=t * N / k / res["discard_s"])
    if "tmpfs_s" in res:
        res["speedup_tmpfs"] = t * N / k / res["tmpfs_s"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tmpfs", default="/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(bench="export_throughput", format="%.8e", results=[bench(N, a.repeats, a.tmpfs) for N in a.rows])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
