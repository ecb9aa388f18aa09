"""Times the mutators of a sample set of 1e7 x 50 fp64 values with integer weights, each three ways in one process on one
machine: the native call alone (gd_select_samples / gd_set_weights), the whole MCSamples method, and the host route the
method took before -- numpy indexing of the host array, then gd_upload of the result, from pageable memory (what numpy
returns) and from page-locked memory -- plus a gd_memcpy_d2d of the bytes the native call reads and writes, as its roof.

    python scripts/bench_select.py [--rows 10000000] [--cols 50] [--calls 3] [--out profiles/select_throughput.json]

Every timed call starts from the same resident set (gd_clone_samples of a master context, a copy() of a master object, both
outside the timed region) and is timed from the host until it has returned, which is when the new set is complete.  Native
calls and methods: one warm-up, then ``--calls`` timed calls, medians reported; the host route: ``--host-calls`` calls (default
1, it takes seconds).  No number is gated but one: on every row the native call must beat the gd_upload of its result from
page-locked memory in the same run (exit status 1 otherwise)."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LINE_DOUBLES = 16  # a 128-byte line: what the gather fetches at most per kept row and column


def ms_of(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=50)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from getdist_amd import devarray
    from getdist_amd._lib import Context
    from getdist_amd.mcsamples import MCSamples

    N, n = a.rows, a.cols
    feeder = Context(0)
    S = feeder.pinned_block((N, n))  # page-locked, row-major
    rng = np.random.default_rng(20261020)
    for r0 in range(0, N, 1 << 20):
        S[r0:r0 + (1 << 20)] = rng.random(S[r0:r0 + (1 << 20)].shape)
    w = rng.integers(1, 5, N).astype(np.float64)
    ll = 0.5 * np.sum((S[:, :3] - 0.5)**2, axis=1) * 12.0
    names = ["p%d" % j for j in range(n)]
    print("samples: %d x %d, %.2f GB" % (N, n, S.nbytes / 1e9), flush=True)

    # the master object, built from a device array (no host mirror), and the master context the native calls clone
    block = feeder.alloc(S.nbytes)
    block.from_host(S)
    dev = devarray.DevArray(block.ptr, (N, n), (n, 1), devarray.GD_DT_F64, owner=block)
    master = MCSamples(samples=dev, weights=w, loglikes=ll, names=names, settings=dict(min_weight_ratio=-1))
    assert not master._host_mirror_ready
    block.free()
    with_fixed = master.copy()
    with_fixed.addDerived(np.full(N, 0.25), "fixed")
    work, up = Context(0), Context(0)
    pinned_result = feeder.pinned_block((N, n + 1))
    spare_a, spare_b = feeder.alloc(S.nbytes), feeder.alloc(S.nbytes)
    up.upload(S, w)  # (warm: the first upload of a process pays for its set-up)

    m50, m01 = rng.random(N) < 0.5, rng.random(N) < 0.01
    mexpr = S[:, 0] > 0.7
    burn = int(round(N * 0.3))
    buf, K_thin = master.ctx.thin_rows(0, N, 10, True, int(w.sum()) // 10 + 2)
    thin_ix = buf.to_host((K_thin,), dtype=np.int32).astype(np.int64)
    wt_rows, wt_counts = np.unique(thin_ix, return_counts=True)
    extra = 0.25 * np.cos(np.arange(N) * 0.37) + 0.3
    w_reweighted = w * np.exp(-(extra - extra.min()))
    w_cooled = w * np.exp(-(ll * 2.0 - ll) - (ll.min() * (1 - 2.0)))
    derived = S[:, 0] * S[:, 1] + 1.0
    keep49 = [c for c in range(n) if c != 7]

    def expr(mc):
        p = mc.getDeviceParams()
        return p.p0 * p.p1 + 1.0

    # name -> (source object, method, native call on ``work``, host indexing -> (samples, weights), K, columns out)
    rows = {
        "filter_p50": (master, lambda mc: mc.filter(m50), lambda: work.select_samples(rows=("mask", m50)), lambda: (S[m50, :], w[m50])),
        "filter_p01": (master, lambda mc: mc.filter(m01), lambda: work.select_samples(rows=("mask", m01)), lambda: (S[m01, :], w[m01])),
        "filter_expr": (master, lambda mc: mc.filter(mc.getDeviceParams().p0 > 0.7), lambda: work.select_samples(rows=("mask", mexpr)),
                        lambda: (S[mexpr, :], w[mexpr])),
        "removeBurn_0.3": (master, lambda mc: mc.removeBurn(0.3), lambda: work.select_samples(rows=("range", burn, N)),
                           lambda: (S[burn:, :], w[burn:])),
        "thin_10": (master, lambda mc: mc.thin(10), lambda: work.select_samples(rows=("rows", buf, K_thin), weights="unit"),
                    lambda: (S[thin_ix, :], None)),
        "weighted_thin_10": (master, lambda mc: mc.weighted_thin(10),
                             lambda: work.select_samples(rows=("rows", wt_rows), weights=wt_counts.astype(np.float64)),
                             lambda: (S[wt_rows, :], wt_counts.astype(np.float64))),
        # (the method drops the constant column appended to ``with_fixed``; the native call and the host route drop one of the 50)
        "deleteFixedParams": (with_fixed, lambda mc: mc.deleteFixedParams(), lambda: work.select_samples(keep_cols=keep49),
                              lambda: (np.delete(S, [7], 1), w)),
        "addDerived_expr": (master, lambda mc: mc.addDerived(expr(mc), "d"), lambda: work.select_samples(append=("slot", 0)),
                            None),  # (host route below: the Fortran-order array of the method)
        # (no indexing on the host route of these two: the whole array was uploaded again with the new weights)
        "reweightAddingLogLikes": (master, lambda mc: mc.reweightAddingLogLikes(extra), lambda: work.set_weights(w_reweighted),
                                   lambda: (pageable(), w_reweighted)),
        "cool_2": (master, lambda mc: mc.cool(2.0), lambda: work.set_weights(w_cooled), lambda: (pageable(), w_cooled)),
    }

    copies = {}

    def pageable():
        if "S" not in copies:
            copies["S"] = np.array(S)
        return copies["S"]

    def add_derived_host():
        new = np.empty((N, n + 1), dtype=np.float64, order="F")
        new[:, :n] = S
        new[:, n] = derived
        return new, w

    def d2d_ms(nbytes):
        nbytes = int(min(nbytes, S.nbytes)) // 16 * 16
        out = []
        for k in range(a.calls + 1):
            t, _ = ms_of(lambda: (feeder.lib.gd_memcpy_d2d(feeder.h, spare_b.ptr, spare_a.ptr, nbytes), feeder.sync()))
            out.append(t)
        return float(np.median(out[1:]))

    res = dict(rows=N, cols=n, bytes=int(S.nbytes), calls=a.calls, host_calls=a.host_calls, table={})
    ok = True
    for name, (source, method, native, host_index) in rows.items():
        weights_only = name in ("reweightAddingLogLikes", "cool_2")
        t_native, t_method = [], []
        for k in range(a.calls + 1):
            work.clone_samples(master.ctx)
            t, _ = ms_of(native)
            t_native.append(t)
        K, n_out = work.N, work.n
        for k in range(a.calls + 1):
            twin = source.copy()
            t, _ = ms_of(lambda: method(twin))
            t_method.append(t)
            assert weights_only or not twin._host_mirror_ready
            assert (twin.ctx.N, twin.ctx.n) == (K, n_out + (1 if source is with_fixed else 0)), (name, twin.ctx.N, twin.ctx.n, K, n_out)
            twin.ctx.close()
        t_index, t_pageable, t_pinned = [], [], []
        if weights_only:
            pageable()  # (made outside the timed region)
        for k in range(a.host_calls):
            ti, (new, new_w) = ms_of(host_index or add_derived_host)
            tp, _ = ms_of(lambda: up.upload(new, new_w))
            assert (up.N, up.n) == (K, n_out)
            if new.flags.f_contiguous and not new.flags.c_contiguous:
                landing = pinned_result.reshape(-1)[:new.size].reshape(new.shape, order="F")
            else:
                landing = pinned_result.reshape(-1)[:new.size].reshape(new.shape)
            landing[...] = new
            del new
            tq, _ = ms_of(lambda: up.upload(landing, new_w))
            t_index.append(ti), t_pageable.append(tp), t_pinned.append(tq)
        if weights_only:  # reads and writes the weight column only
            moved = 2 * N * 8
        else:
            w_out = 0 if name == "thin_10" else 1
            contiguous = name in ("removeBurn_0.3", "deleteFixedParams", "addDerived_expr")
            read = (K if contiguous else min(N, K * LINE_DOUBLES)) * (n_out + w_out) * 8
            moved = read + K * (n_out + w_out) * 8
        roof = d2d_ms(moved / 2)
        row = dict(rows_out=int(K), cols_out=int(n_out), native_ms=t_native[1:], native_ms_median=float(np.median(t_native[1:])),
                   method_ms=t_method[1:], method_ms_median=float(np.median(t_method[1:])),
                   host_index_ms_median=float(np.median(t_index)), upload_pageable_ms_median=float(np.median(t_pageable)),
                   upload_pinned_ms_median=float(np.median(t_pinned)), bytes_read_plus_written=int(moved), memcpy_d2d_roof_ms=roof)
        row["host_route_ms"] = row["host_index_ms_median"] + row["upload_pageable_ms_median"]
        row["host_route_over_native"] = row["host_route_ms"] / row["native_ms_median"]
        row["host_route_over_method"] = row["host_route_ms"] / row["method_ms_median"]
        row["fraction_of_d2d_rate"] = roof / row["native_ms_median"]
        row["native_beats_pinned_upload"] = bool(row["native_ms_median"] < row["upload_pinned_ms_median"])
        ok = ok and row["native_beats_pinned_upload"]
        res["table"][name] = row
        print("%-24s native %8.2f ms  method %8.2f ms  host index %8.1f + upload %7.1f (pageable) / %7.1f (page-locked) ms  "
              "roof %6.2f ms (%.2f of the device-copy rate)  %s"
              % (name, row["native_ms_median"], row["method_ms_median"], row["host_index_ms_median"], row["upload_pageable_ms_median"],
                 row["upload_pinned_ms_median"], roof, row["fraction_of_d2d_rate"], "" if row["native_beats_pinned_upload"] else "SLOWER"),
              flush=True)
        if a.out:  # (kept current: a long run leaves what it has measured)
            with open(a.out, "w") as f:
                json.dump(dict(command="python scripts/bench_select.py", result=res), f, indent=1)
    res["every_native_call_beats_the_pinned_upload_of_its_result"] = ok
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(command="python scripts/bench_select.py", result=res), f, indent=1)
    buf.free()
    for c in (work, up):
        c.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
