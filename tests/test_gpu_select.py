"""GPU tier of the device-side edits of a sample set (gd_select_samples, gd_set_weights, and the mutators of chains.py that
go through them).  The yardstick is always numpy indexing of the host arrays followed by a fresh gd_upload into a second
context: resident columns, spare columns and weights bit-equal, the integral flag and gd_weight_stats equal.  Shapes sit at
the edges of the tile of the row-list passes (GD_SEL_TILE rows), of the 512-row leading dimension and of the column chunk of
the gather, not at the workload's size."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import devinput_cases as dc  # noqa: E402
import golden_util as gu  # noqa: E402
import select_cases as sc  # noqa: E402
from test_gpu_compose import device_rows  # noqa: E402
from test_gpu_devinput import TOL_GRID, TOL_MOMENTS, assert_same_mcsamples, assert_same_resident  # noqa: E402

pytestmark = pytest.mark.gpu

from getdist_amd._lib import GD_SEL_TILE as T  # noqa: E402

SHAPES_N = [1, 511, 512, 513, T - 1, T, T + 1, 3 * T + 17]
SHAPES_n = [1, 3, 33]


@pytest.fixture(scope="module")
def ctxs():
    """(feeder: the second context device masks and row lists are filled through, edited context, yardstick context)"""
    from getdist_amd._lib import Context

    three = Context(0), Context(0), Context(0)
    yield three
    for c in three:
        c.close()


def weights_of(kind, N, seed=3):
    r = np.random.default_rng(seed)
    if kind == "none":
        return None
    if kind == "bytes":
        return r.integers(0, 256, N).astype(float)
    if kind == "one_300":  # a single multiplicity above 255: no byte copy until the selection removes that row
        w = r.integers(1, 200, N).astype(float)
        w[N // 2] = 300.0
        return w
    return r.gamma(2.0, 1.0, N)


def on_device(feeder, a):
    buf = feeder.alloc(max(a.nbytes, 8))
    buf.from_host(np.ascontiguousarray(a))
    return buf


def check(ctxs, S, w, rows, index, keep=None, append=None, weights="keep", append_values=None):
    """upload (S, w), select, and compare with the upload of the numpy-indexed arrays.  ``index``: what numpy takes for the
    rows; ``append_values``: the N values of the appended column (``append`` itself may name a spare slot)."""
    _, dev, host = ctxs
    dev.upload(S, w)
    if isinstance(append, tuple):
        dev.set_extra_column(append[1], append_values)
    K = dev.select_samples(rows=rows, keep_cols=keep, append=append, weights=weights)
    want = S[index] if keep is None else S[index][:, keep]
    if append is not None:
        want = np.column_stack([want, np.asarray(append_values)[index]])
    if isinstance(weights, str):
        want_w = w[index] if (weights == "keep" and w is not None) else None
    else:
        want_w = np.asarray(weights, dtype=float)
    host.upload(np.ascontiguousarray(want), want_w)
    assert K == len(want)
    n64, nn = C.c_int64(), C.c_int64()
    dev._check(dev.lib.gd_num_rows(dev.h, C.byref(n64), C.byref(nn)))
    assert (n64.value, nn.value) == want.shape
    assert_same_resident(dev, host)


def masks(N, seed=11):
    r = np.random.default_rng(seed)
    out = {"all": np.ones(N, dtype=bool), "first_row": np.arange(N) == 0, "last_row": np.arange(N) == N - 1,
           "alternating": np.arange(N) % 2 == 1, "first_half": np.arange(N) < (N + 1) // 2,
           "empty_tiles_then_full": np.arange(N) >= (N // T // 2 + (1 if N > T else 0)) * T if N > 1 else np.ones(N, dtype=bool),
           "p50": r.random(N) < 0.5, "p01": r.random(N) < 0.01}
    return {k: m for k, m in out.items() if m.any()}


@pytest.mark.parametrize("n", SHAPES_n)
@pytest.mark.parametrize("N", SHAPES_N)
def test_masks(ctxs, N, n):
    S, w = dc.values(N, n), weights_of("real", N)
    for where, (name, m) in enumerate(masks(N).items()):
        if where % 2:
            check(ctxs, S, w, ("mask", on_device(ctxs[0], m.astype(np.uint8) * 7)), m)  # any non-zero byte keeps the row
        else:
            check(ctxs, S, w, ("mask", m), m)


@pytest.mark.parametrize("n", SHAPES_n)
@pytest.mark.parametrize("N", SHAPES_N)
def test_row_lists(ctxs, N, n):
    S, w = dc.values(N, n), weights_of("bytes", N)
    r = np.random.default_rng(N + n)
    lists = [np.arange(N), np.arange(N)[::-1], np.sort(r.integers(0, N, max(N // 2, 1))), r.integers(0, N, 2 * N + 3)]
    for k, ix in enumerate(lists):
        ix = ix.astype(np.int32)
        check(ctxs, S, w, ("rows", on_device(ctxs[0], ix), len(ix)) if k % 2 else ("rows", ix), ix)
        check(ctxs, S, w, ("rows", ix) if k % 2 else ("rows", on_device(ctxs[0], ix), len(ix)), ix)


@pytest.mark.parametrize("N", SHAPES_N)
def test_ranges(ctxs, N):
    S, w = dc.values(N, 3), weights_of("real", N)
    for lo, hi in {(0, N), (N // 3, N), (N // 3, max(N - 5, N // 3 + 1)), (min(7, N - 1), min(519, N))}:
        check(ctxs, S, w, ("range", lo, hi), slice(lo, hi))
    check(ctxs, S, None, None, slice(None))


@pytest.mark.parametrize("rows", ["all", "mask"])
def test_columns(ctxs, rows):
    N, n = T + 1, 33
    S, w = dc.values(N, n), weights_of("bytes", N)
    m = np.random.default_rng(4).random(N) < 0.5
    sel, index = (None, slice(None)) if rows == "all" else (("mask", m), m)
    for keep in (list(range(1, n)), list(range(n - 1)), [c for c in range(n) if c != 16], [0, 8, 9, 32], [5]):
        check(ctxs, S, w, sel, index, keep=keep)
    vec = np.cos(np.arange(N) * 0.01)
    check(ctxs, S, w, sel, index, append=vec, append_values=vec)
    check(ctxs, S, w, sel, index, append=("slot", 2), append_values=vec)
    check(ctxs, S, w, sel, index, keep=[0, 3], append=("slot", 0), append_values=vec)
    check(ctxs, S, None, sel, index, keep=[2], append=vec, append_values=vec, weights="unit")


@pytest.mark.parametrize("kind", ["none", "bytes", "one_300", "real"])
def test_weight_kinds(ctxs, kind):
    N = 2 * T + 5
    S, w = dc.values(N, 3), weights_of(kind, N)
    m = np.random.default_rng(6).random(N) < 0.5
    m[N // 2] = False  # the row of the multiplicity of 300 goes: byte multiplicities exactly as after a fresh upload
    check(ctxs, S, w, ("mask", m), m)
    assert ctxs[1].weights_integral() == (kind != "real")
    check(ctxs, S, w, ("mask", m), m, weights="unit")
    new = np.random.default_rng(7).integers(1, 9, int(m.sum())).astype(float)
    check(ctxs, S, w, ("mask", m), m, weights=new)
    ix = np.flatnonzero(m).astype(np.int32)
    check(ctxs, S, w, ("rows", ix), ix, weights=new)
    check(ctxs, S, w, ("range", 3, 3 + len(new)), slice(3, 3 + len(new)), weights=new)


@pytest.mark.parametrize("kind", ["bytes", "real", "none"])
def test_weight_threshold(ctxs, kind):
    N = 3 * T + 17
    S, w = dc.values(N, 3), weights_of(kind, N)
    if w is None:
        check(ctxs, S, None, ("weight_gt", 0.5), slice(None))
        return
    u = np.unique(w)
    for thr in (u[len(u) // 2], 0.0, u[-2]):  # (equal to one of the weights: the rows that carry it go, w > thr)
        check(ctxs, S, w, ("weight_gt", thr), w > thr)


def test_more_tiles_than_one_scan_pass(ctxs):
    N = 1024 * T + 3 * T + 5  # 1028 tile counts: k_tile_scan takes 1024 per pass
    r = np.random.default_rng(12)
    S, w = r.standard_normal((N, 2)), r.integers(0, 4, N).astype(float)
    m = r.random(N) < 0.5
    m[:5 * T] = False
    check(ctxs, S, w, ("mask", m), m)
    check(ctxs, S, w, ("weight_gt", 1.0), w > 1.0)


@pytest.mark.parametrize("unique_mode", [0, 1])
def test_row_list_straight_from_thin_rows(ctxs, unique_mode):
    _, dev, _ = ctxs
    N = 3 * T + 17
    S = dc.values(N, 3)
    w = np.random.default_rng(8).integers(0, 4, N).astype(float)
    factor = 5 if unique_mode else 2
    dev.upload(S, w)
    buf, K = dev.thin_rows(0, N, factor, unique_mode, int(w.sum()) // factor + 2)
    ix = buf.to_host((K,), dtype=np.int32)
    assert np.array_equal(ix, sc.thin_indices(factor, w))
    check(ctxs, S, w, ("rows", buf, K), ix, weights="unit")
    buf.free()


def test_set_weights(ctxs):
    _, dev, host = ctxs
    N = T + 513
    S = dc.values(N, 5)
    dev.upload(S, weights_of("real", N))
    for kind in ("bytes", "none", "real", "one_300", "bytes", "none"):
        w = weights_of(kind, N, seed=len(kind))
        dev.set_weights(w)
        host.upload(S, w)
        assert_same_resident(dev, host)  # columns untouched, weights, flags and weight_stats as after a fresh upload
        assert dev.weights_integral() == host.weights_integral()
        if kind == "bytes":  # a following thinning uses the new weights (the cumulative weights are rebuilt)
            buf, K = dev.thin_rows(0, N, 300, 1, int(w.sum()) // 300 + 2)
            assert np.array_equal(buf.to_host((K,), dtype=np.int32), sc.thin_indices(300, w))
            buf.free()
            assert dev.cov()[1].tolist() == host.cov()[1].tolist()
        if kind != "real":  # the linear-bucket select: the bucket columns of the previous weight mode are gone
            mm = np.stack([S[:, [0, 4]].min(axis=0), S[:, [0, 4]].max(axis=0)], axis=1)
            targets = np.array([[0.16, 0.5], [0.5, 0.84]]) * (N if w is None else w.sum())
            assert dev.quantiles([0, 4], targets, minmax=mm).tolist() == host.quantiles([0, 4], targets, minmax=mm).tolist()


# ---- refusals (only the selections that turn out empty reach the row-list kernels; none reaches the gather) -----------------
def test_refusals_leave_the_previous_set_resident(ctxs):
    from getdist_amd._lib import GD_ERR_BADARG, GD_SEL_MASK_U8, GD_SEL_RANGE, GD_SEL_ROWS_I32, GD_SEL_W_REPLACE, Context, GdSelection

    _, dev, _ = ctxs
    before, wb = dc.values(33, 4), weights_of("real", 33)
    dev.upload(before, wb)
    keep_bad = [np.array(v, dtype=np.int32) for v in ([0, 4], [-1, 2], [2, 1], [1, 1])]
    rows_bad = [np.array(v, dtype=np.int32) for v in ([0, 33], [-1])]
    none = np.zeros(33, dtype=np.uint8)
    neww = np.ones(5)

    def call(ctx=dev, **kw):
        sel = GdSelection()
        for k, v in kw.items():
            setattr(sel, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        return ctx.lib.gd_select_samples(ctx.h, C.byref(sel), None)

    empty, borrower = Context(0), Context(0)
    borrower.attach(dev)
    cases = [call(ctx=empty), call(ctx=borrower), borrower.lib.gd_set_weights(borrower.h, None), empty.lib.gd_set_weights(empty.h, None)]
    for lo, hi in ((-1, 5), (0, 34), (5, 5), (9, 3), (34, 40)):
        cases.append(call(row_kind=GD_SEL_RANGE, lo=lo, hi=hi))
    cases += [call(keep=k, m=len(k)) for k in keep_bad]
    cases += [call(keep=keep_bad[0], m=0), call(row_kind=9), call(append_kind=7), call(append_kind=2, append_slot=4), call(append_kind=1),
              call(weight_kind=5), call(weight_kind=GD_SEL_W_REPLACE), call(weight_kind=GD_SEL_W_REPLACE, new_weights=neww, K=5),
              call(row_kind=GD_SEL_MASK_U8), call(row_kind=GD_SEL_ROWS_I32, K=2)]
    cases += [call(row_kind=GD_SEL_ROWS_I32, rows=r, K=len(r)) for r in rows_bad]
    cases += [call(row_kind=GD_SEL_ROWS_I32, rows=rows_bad[0], K=0), call(row_kind=GD_SEL_MASK_U8, rows=none),
              call(row_kind=3, thr=float(wb.max())), call(row_kind=3, thr=float("nan")),
              call(row_kind=GD_SEL_MASK_U8, rows=np.ones(33, dtype=np.uint8), weight_kind=GD_SEL_W_REPLACE, new_weights=neww, K=5)]
    for k, got in enumerate(cases):
        assert got == GD_ERR_BADARG, k
    assert b"no rows selected" in dev.lib.gd_last_error(dev.h) or b"number of new weights" in dev.lib.gd_last_error(dev.h)
    assert call(row_kind=GD_SEL_MASK_U8, rows=none) == GD_ERR_BADARG and b"no rows selected" in dev.lib.gd_last_error(dev.h)
    # auxiliary weights selected: both calls refuse
    dev.aux_weights(np.ones(33))
    dev.select_weights(1)
    assert call() == GD_ERR_BADARG and dev.lib.gd_set_weights(dev.h, None) == GD_ERR_BADARG and dev.lib.gd_last_error(dev.h)
    dev.select_weights(0)
    borrower.close(), empty.close()
    n64, nn = C.c_int64(), C.c_int64()
    dev._check(dev.lib.gd_num_rows(dev.h, C.byref(n64), C.byref(nn)))
    assert (n64.value, nn.value) == (33, 4)
    for j in range(4):
        assert np.array_equal(device_rows(dev, j), before[:, j])
    assert np.array_equal(device_rows(dev, -2), wb)


# ---- the mutators of an MCSamples ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feeder(ctxs):
    return ctxs[0]


@pytest.mark.parametrize("source", ["device_arrays", "host_arrays"])
@pytest.mark.parametrize("kind", ["single", "chains"])
@pytest.mark.parametrize("name", list(sc.MUTATORS))
def test_mutator_equals_a_fresh_object_of_the_numpy_edit(feeder, name, kind, source):
    from getdist_amd.mcsamples import MCSamples

    inp = sc.inputs(kind)
    dev = sc.make(MCSamples, inp, (lambda a: dc.DevBuf(a, feeder)) if source == "device_arrays" else None)
    want = sc.expected(MCSamples, name, inp)
    apply, _, replaces_rows = sc.MUTATORS[name]
    apply(dev)
    if replaces_rows or source == "device_arrays":
        assert not dev._host_mirror_ready  # (on the parent commit every mutator forms or keeps the host mirror)
    assert_same_mcsamples(dev, want)
    assert dev.ranges.lower == want.ranges.lower and dev.ranges.upper == want.ranges.upper
    assert np.array_equal(dev.getMeans(), want.getMeans()) and np.array_equal(dev.fullcov, want.fullcov)
    assert gu.relerr(dev.cov(), want.cov()) < TOL_MOMENTS
    a, b = dev.get1DDensity("y"), want.get1DDensity("y")
    assert np.max(np.abs(a.P - b.P)) < TOL_GRID * np.max(b.P)
    a, b = dev.get2DDensity("x", "y"), want.get2DDensity("x", "y")
    assert np.max(np.abs(a.P - b.P)) < TOL_GRID * np.max(b.P)
    if replaces_rows or source == "device_arrays":
        assert not dev._host_mirror_ready
    got = dev.samples
    assert dev._host_mirror_ready and np.array_equal(got, want.samples)
    dev.ctx.close(), want.ctx.close()
