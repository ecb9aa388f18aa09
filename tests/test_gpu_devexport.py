"""GPU tier of device-array output (gd_export_device, getDeviceSamples / getDeviceWeights, devarray.DeviceArray).  Every case
writes into a view of a larger device block that was filled with a sentinel pattern through a second context, downloads
the WHOLE block and compares it bit for bit with the same block made on the host: numpy indexing of the host values,
narrowed with ``astype`` (bf16: the exact model of devexport_cases), inside the view, the sentinel everywhere else.  Shapes
sit at the edges of the kernel paths (the slab's R rows, the 16-byte vector of each type, the 32-wide tile), not at the
workload's size.  Refusals use arguments that never reach a kernel."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import devexport_cases as xc  # noqa: E402
import devinput_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.float16, "bfloat16"]
UINT = {8: np.uint64, 4: np.uint32, 2: np.uint16}
SENTINEL = 0xA5C3A5C3A5C3A5C3
PAD = 8  # elements of sentinel in front of and behind every view


def itemsize(dtype):
    return 2 if dtype == "bfloat16" else np.dtype(dtype).itemsize


def code_of(dtype):
    from getdist_amd import devarray

    return devarray.dtype_code(dtype)


@pytest.fixture(scope="module")
def ctxs():
    """(feeder: the second context the destination blocks are filled and read through, the context under test)"""
    from getdist_amd._lib import Context

    two = Context(0), Context(0)
    yield two
    for c in two:
        c.close()


LAYOUTS = {  # name -> (first element, row stride, column stride) in elements, for K rows and m columns
    "C": lambda K, m: (PAD, m, 1),
    "F": lambda K, m: (PAD, 1, K),
    "row_gap": lambda K, m: (PAD, m + 3, 1),           # the three elements behind every row must stay
    "odd_base": lambda K, m: (PAD + 1, m, 1),          # element-aligned, never 16-byte aligned
    "transposed_gaps": lambda K, m: (PAD, 2, 2 * K + 4),  # neither stride is 1: the tile path
}


class Target:
    """a device block of sentinel bits and the (K, m) view of it that an export writes"""

    def __init__(self, feeder, K, m, dtype, layout):
        from getdist_amd import devarray

        self.size = itemsize(dtype)
        first, rs, cs = LAYOUTS[layout](K, m)
        self.index = first + np.add.outer(np.arange(K) * rs, np.arange(m) * cs)  # flat element index of (k, c)
        total = int(self.index.max() if self.index.size else first) + 1 + PAD
        self.bits = np.full(total, SENTINEL & ((1 << (8 * self.size)) - 1), dtype=UINT[self.size])
        self.buf = feeder.alloc(self.bits.nbytes)
        self.buf.from_host(self.bits)
        self.desc = devarray.DevArray(self.buf.ptr + first * self.size, (K, m), (rs, cs), code_of(dtype), owner=self.buf)

    def download(self):
        return self.buf.to_host((self.bits.size,), dtype=self.bits.dtype)

    def expected(self, narrowed_bits):
        want = self.bits.copy()
        want[self.index.reshape(-1)] = narrowed_bits.reshape(-1)
        return want

    def free(self):
        self.buf.free()


def check(ctxs, values, rows, cols, dtype, layout, want=None):
    """export ``rows`` x ``cols`` into a fresh target and compare the whole block; ``values``: the (K, m) float64 values
    numpy selects (``want``: their narrowed bits, when the caller has them already)"""
    feeder, ctx = ctxs
    K, m = values.shape
    t = Target(feeder, K, m, dtype, layout)
    try:
        assert ctx.export_device(rows=rows, cols=cols, dest=t.desc) == K
        got = t.download()
        assert np.array_equal(got, t.expected(xc.narrowed(values, dtype) if want is None else want)), (dtype, layout)
    finally:
        t.free()


def resident(ctx, N, n, seed=3, weights=None):
    """upload (N, n) values with the targeted values of the conversions among them; returns them with the spare columns"""
    x = xc.sample_values(N, n, seed)
    ctx.upload(x, weights)
    return np.hstack([x, np.zeros((N, ctx.EXTRA_COLS))])


# ---- shapes, types, layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 33, 50, 65])
@pytest.mark.parametrize("N", [1, 7, 9, 127, 128, 129, 1025])
def test_all_rows_every_type_and_layout(ctxs, N, n):
    x = resident(ctxs[1], N, n, seed=N * 100 + n)
    cols = list(range(n))
    for dtype in DTYPES:
        want = xc.narrowed(x[:, :n], dtype)
        for layout in LAYOUTS:
            check(ctxs, x[:, :n], None, cols, dtype, layout, want)


@pytest.mark.parametrize("lo,hi", [(3, 900), (129, 130), (1, 1025), (128, 385), (511, 511)])
def test_ranges_with_odd_and_even_offsets(ctxs, lo, hi):
    x = resident(ctxs[1], 1025, 50)
    cols = list(range(50))
    for dtype in DTYPES:
        want = xc.narrowed(x[lo:hi, :50], dtype)
        for layout in ("C", "F", "row_gap"):
            check(ctxs, x[lo:hi, :50], ("range", lo, hi), cols, dtype, layout, want)


def device_bytes(feeder, a):
    buf = feeder.alloc(max(a.nbytes, 8))
    buf.from_host(a)
    return buf


@pytest.mark.parametrize("where", ["host", "device"])
def test_masks_across_a_tile_boundary(ctxs, where):
    feeder, ctx = ctxs
    x = resident(ctx, 3000, 9)
    r = np.random.default_rng(5)
    cols = [8, 0, 3]
    for mask in (r.random(3000) < 0.5, (np.arange(3000) >= 1020) & (np.arange(3000) < 1030), r.random(3000) < 0.01,
                 np.zeros(3000, bool), np.ones(3000, bool)):
        held = device_bytes(feeder, mask.view(np.uint8)) if where == "device" else None
        rows = ("mask", held if held is not None else mask)
        assert ctx.export_device(rows=rows, cols=cols) == int(mask.sum())  # (a count: nothing to write to)
        for dtype, layout in ((np.float64, "C"), (np.float32, "row_gap"), ("bfloat16", "F"), (np.float16, "transposed_gaps")):
            check(ctxs, x[mask][:, cols], rows, cols, dtype, layout)
        if held is not None:
            held.free()


@pytest.mark.parametrize("where", ["host", "device"])
def test_row_lists_in_any_order_with_repeats(ctxs, where):
    feeder, ctx = ctxs
    x = resident(ctx, 1025, 12)
    index = np.concatenate([np.arange(1024, 0, -3), [7, 7, 7, 0, 1024], np.arange(300)]).astype(np.int32)
    held = device_bytes(feeder, index) if where == "device" else None
    rows = ("rows", held, index.size) if held is not None else ("rows", index)
    cols = list(range(12))
    for dtype, layout in ((np.float64, "C"), (np.float32, "F"), (np.float16, "row_gap"), ("bfloat16", "odd_base")):
        check(ctxs, x[index][:, cols], rows, cols, dtype, layout)
    if held is not None:
        held.free()


def test_columns_with_repeats_and_spare_columns(ctxs):
    _, ctx = ctxs
    x = resident(ctx, 513, 6)
    extra = np.random.default_rng(2).standard_normal(513)
    assert ctx.set_extra_column(1, extra) == 7
    x[:, 7] = extra
    cols = [3, 3, 7, 0, 9, 5, 3]
    for rows, index in ((None, slice(None)), (("range", 1, 512), slice(1, 512)), (("rows", np.array([512, 0, 512])), [512, 0, 512])):
        for dtype, layout in ((np.float64, "C"), (np.float32, "C"), (np.float16, "F"), ("bfloat16", "transposed_gaps")):
            check(ctxs, x[index][:, cols], rows, cols, dtype, layout)


def test_rows_where_a_spare_column_is_not_zero(ctxs):
    _, ctx = ctxs
    x = resident(ctx, 2500, 4)
    flag = (np.random.default_rng(4).random(2500) < 0.3).astype(np.float64)
    flag[::97] = np.nan  # (NaN != 0 holds: what a boolean expression's fetch as bytes gives too)
    col = ctx.set_extra_column(2, flag)
    keep = flag != 0
    check(ctxs, x[keep][:, [0, 3]], ("nonzero", col), [0, 3], np.float32, "C")
    check(ctxs, x[keep][:, [1]], ("nonzero", col), [1], np.float64, "F")


@pytest.mark.parametrize("weighted", [True, False])
def test_weight_column_and_weight_threshold(ctxs, weighted):
    _, ctx = ctxs
    N = 1300
    w = np.random.default_rng(8).gamma(2.0, 1.0, N) if weighted else None
    resident(ctx, N, 3, weights=w)
    hw = w if weighted else np.ones(N)
    mask = np.random.default_rng(9).random(N) < 0.4
    for rows, index in ((None, slice(None)), (("range", 5, 1290), slice(5, 1290)), (("mask", mask), mask),
                        (("rows", np.array([3, 1, 1299, 3])), [3, 1, 1299, 3]), (("weight_gt", 1.5), hw > 1.5),
                        (("weight_gt", 0.5), hw > 0.5)):
        for dtype, layout in ((np.float64, "C"), (np.float32, "odd_base"), (np.float16, "row_gap"), ("bfloat16", "C")):
            check(ctxs, hw[index][:, None], rows, None, dtype, layout)


def test_a_selection_of_nothing(ctxs):
    feeder, ctx = ctxs
    resident(ctx, 600, 5)
    t = Target(feeder, 4, 5, np.float32, "C")
    for rows in (("mask", np.zeros(600, bool)), ("range", 17, 17), ("rows", np.zeros(0, np.int32)), ("weight_gt", 1.0)):
        assert ctx.export_device(rows=rows, cols=list(range(5)), dest=t.desc) == 0
        assert ctx.export_device(rows=rows, cols=list(range(5))) == 0
    assert np.array_equal(t.download(), t.bits)
    t.free()


def test_too_small_a_destination_reports_the_count_and_writes_nothing(ctxs):
    feeder, ctx = ctxs
    resident(ctx, 600, 5)
    mask = np.arange(600) % 3 == 0
    t = Target(feeder, 199, 5, np.float64, "C")
    for rows, K in ((("mask", mask), 200), (None, 600), (("rows", np.arange(200)), 200)):
        with pytest.raises(ValueError, match="199 rows, %d are selected" % K):
            ctx.export_device(rows=rows, cols=list(range(5)), dest=t.desc)
        assert ctx.export_device(rows=rows, cols=list(range(5))) == K
    assert np.array_equal(t.download(), t.bits)
    t.free()


# ---- refusals: none of these can reach a kernel ---------------------------------------------------------------------------
def test_refusals_leave_destination_and_resident_set_alone(ctxs):
    from getdist_amd._lib import GD_ERR_BADARG, GD_ERR_DECLINED, GdExport

    feeder, ctx = ctxs
    x = resident(ctx, 64, 5)
    t = Target(feeder, 64, 5, np.float64, "C")
    cols = np.arange(5, dtype=np.int32)
    pinned = feeder.pinned_array((64, 5))
    pinned[:] = -3.0

    def call(base=t.desc.ptr, capacity=64, rs=5, cs=1, dtype=0, m=5, row_kind=0, lo=0, hi=0, rows=None, K=0, colptr=cols.ctypes.data):
        ex = GdExport()
        ex.row_kind, ex.lo, ex.hi, ex.rows, ex.K, ex.m, ex.cols = row_kind, lo, hi, rows, K, m, colptr
        ex.base, ex.rows_capacity, ex.row_stride, ex.col_stride, ex.dtype = base, capacity, rs, cs, dtype
        count = C.c_int64(-1)
        return ctx.lib.gd_export_device(ctx.h, C.byref(ex), C.byref(count))

    bad_cols = np.array([0, 9, 1, 2, 3], dtype=np.int32)
    bad_rows = np.array([0, 64], dtype=np.int32)
    cases = [
        (call(rs=0), GD_ERR_BADARG),                      # every row at one address
        (call(rs=4), GD_ERR_BADARG),                      # row_stride < m with col_stride 1
        (call(cs=0), GD_ERR_BADARG),
        (call(rs=2, cs=6), GD_ERR_BADARG),                # (3, 0) and (0, 1) share an address
        (call(rs=-5), GD_ERR_DECLINED),
        (call(cs=-1), GD_ERR_DECLINED),
        (call(rs=1 << 40), GD_ERR_BADARG),                # reaches past the allocation
        (call(capacity=1 << 30), GD_ERR_BADARG),           # room for more rows than the allocation holds
        (call(base=t.desc.ptr + 4), GD_ERR_BADARG),       # not aligned to the element
        (call(base=None), GD_ERR_BADARG),
        (call(base=pinned.ctypes.data), GD_ERR_DECLINED),  # page-locked host memory
        (call(dtype=9), GD_ERR_BADARG),
        (call(m=0), GD_ERR_BADARG),
        (call(colptr=bad_cols.ctypes.data), GD_ERR_BADARG),
        (call(row_kind=77), GD_ERR_BADARG),
        (call(row_kind=1, lo=5, hi=65), GD_ERR_BADARG),
        (call(row_kind=1, lo=6, hi=5), GD_ERR_BADARG),
        (call(row_kind=4, rows=bad_rows.ctypes.data, K=2), GD_ERR_BADARG),
        (call(capacity=-1), GD_ERR_BADARG),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
        assert ctx.lib.gd_last_error(ctx.h)
    assert np.array_equal(t.download(), t.bits) and np.all(pinned == -3.0)
    for j in range(5):
        assert np.array_equal(ctx.read_column(j).view(np.uint64), x[:, j].view(np.uint64))
    with pytest.raises(ValueError, match="plain device memory"):
        from getdist_amd import devarray

        ctx.export_device(cols=[0], dest=devarray.DevArray(pinned.ctypes.data, (64, 1), (5, 1), devarray.GD_DT_F64))
    t.free()


# ---- the sample-set methods --------------------------------------------------------------------------------------------------
def test_end_to_end_on_a_set_built_from_a_device_buffer(ctxs):
    from getdist_amd.mcsamples import MCSamples

    feeder, _ = ctxs
    r = np.random.default_rng(31)
    x = r.standard_normal((4099, 6)) * np.array([1.0, 2.0, 0.1, 5.0, 1.0, 3.0]) + np.array([0.0, 1.0, 0.3, 70.0, 0.0, 0.0])
    names = ["x%d" % k for k in range(6)]
    mc = MCSamples(samples=dc.DevBuf(x, feeder), names=names)
    assert not mc._host_mirror_ready
    p = mc.getDeviceParams()
    xp, fp = np.linspace(-4.0, 4.0, 33), np.cos(np.linspace(-4.0, 4.0, 33))
    items = ["x3", 1, p.x1 * np.sqrt(np.abs(p.x2) / 0.3), np.interp(p.x0, xp, fp), "x5", p.x4 + 1.0, p.x4 - 1.0, p.x4 * 2.0, p.x4 * 0.5]
    got = mc.getDeviceSamples(items, rows=p.x0 > 0.25, dtype=np.float32)
    keep = x[:, 0] > 0.25
    want = np.column_stack([x[:, 3], x[:, 1], x[:, 1] * np.sqrt(np.abs(x[:, 2]) / 0.3), np.interp(x[:, 0], xp, fp), x[:, 5], x[:, 4] + 1.0,
                            x[:, 4] - 1.0, x[:, 4] * 2.0, x[:, 4] * 0.5])[keep].astype(np.float32)
    assert got.shape == want.shape and np.array_equal(got.numpy(), want)
    one = mc.getDeviceSamples("x2", rows=slice(1, 4000), dtype="bfloat16", order="F")
    assert np.array_equal(one.numpy(), xc.bf16_model(x[1:4000, 2]))
    assert np.array_equal(mc.getDeviceWeights(rows=[-1, 5]).numpy(), np.ones(2))
    full = mc.getDeviceSamples(order="F")
    assert full.strides == (1, 4099) and np.array_equal(full.numpy(), x)
    again = MCSamples(samples=full, names=names)  # an export fed back in
    assert not again._host_mirror_ready and np.array_equal(again.ctx.read_column(4), x[:, 4])
    assert not mc._host_mirror_ready
    twin = mc.copy()
    assert np.array_equal(twin.getDeviceSamples(["x1", "x0"], rows=slice(10, 20)).numpy(), x[10:20, [1, 0]])
    again.ctx.close(), twin.ctx.close(), mc.ctx.close()


def test_out_views_and_refused_memory(ctxs):
    from getdist_amd import devarray
    from getdist_amd.mcsamples import MCSamples

    feeder, _ = ctxs
    x = np.random.default_rng(32).standard_normal((700, 4))
    w = np.random.default_rng(33).integers(1, 4, 700).astype(float)
    mc = MCSamples(samples=x, weights=w, names=list("abcd"))
    t = Target(feeder, 700, 4, np.float16, "row_gap")
    assert mc.getDeviceSamples(out=t.desc) is t.desc
    assert np.array_equal(t.download(), t.expected(xc.narrowed(x, np.float16)))
    t.free()
    t = Target(feeder, 300, 1, np.float32, "row_gap")
    vec = devarray.DevArray(t.desc.ptr, (300,), (4,), t.desc.dtype, owner=t.buf)
    mc.getDeviceWeights(rows=slice(100, 400), out=vec)
    assert np.array_equal(t.download(), t.expected(xc.narrowed(w[100:400], np.float32)))
    pinned = feeder.pinned_array((700, 4))
    pinned[:] = -3.0
    with pytest.raises(ValueError, match="plain device memory with non-negative strides"):
        mc.getDeviceSamples(out=devarray.DevArray(pinned.ctypes.data, (700, 4), (4, 1), devarray.GD_DT_F64))
    with pytest.raises(ValueError, match="plain device memory with non-negative strides"):
        mc.getDeviceSamples("a", rows=slice(100, 400), out=devarray.DevArray(t.desc.ptr + 299 * 16, (300,), (-4,), devarray.GD_DT_F32))
    assert np.all(pinned == -3.0) and np.array_equal(t.download(), t.expected(xc.narrowed(w[100:400], np.float32)))
    t.free()
    mc.ctx.close()


# ---- lifetime --------------------------------------------------------------------------------------------------------------
def test_an_export_outlives_mutators_and_its_context():
    from getdist_amd.mcsamples import MCSamples

    x = np.random.default_rng(41).standard_normal((3000, 5))
    w = np.random.default_rng(42).integers(1, 4, 3000).astype(float)
    mc = MCSamples(samples=x, weights=w, names=list("abcde"))
    p = mc.getDeviceParams()
    a = mc.getDeviceSamples(["a", "c", p.b * 2.0], rows=slice(1, 2900), dtype=np.float32)
    wa = mc.getDeviceWeights()
    want, want_w = np.column_stack([x[1:2900, 0], x[1:2900, 2], x[1:2900, 1] * 2.0]).astype(np.float32), w.copy()
    mc.filter(p.a > 0.0)
    assert np.array_equal(a.numpy(), want)
    mc.removeBurn(100)
    mc.ctx.close()
    del mc
    assert np.array_equal(a.numpy(), want) and np.array_equal(wa.numpy(), want_w)


def test_the_block_is_returned_when_the_last_reference_goes(ctxs):
    """Free device memory comes back within one allocation granule.  The granule is not guessed: the block is sized a few
    bytes over a multiple of 64 MiB, so what the allocator takes beyond the bytes asked for (free before - free with the
    block - bytes) is its rounding for THIS block, and the granule it rounds to is at most the next power of two of that."""
    from getdist_amd import devarray

    _, ctx = ctxs
    resident(ctx, 64, 2)
    nbytes = (64 << 20) + 4104
    index = np.full(nbytes // 8, 5, dtype=np.int32)
    warm = devarray.DeviceArray.allocate(ctx, (nbytes // 8,), devarray.GD_DT_F64)  # (whatever the first round sets up: the
    ctx.export_device(rows=("rows", index), cols=[1], dest=warm.describe().as2d())  # context's scratch for the row list)
    warm.numpy()
    del warm
    start = ctx.device_info()["hbm_free"]
    a = devarray.DeviceArray.allocate(ctx, (nbytes // 8,), devarray.GD_DT_F64)
    ctx.export_device(rows=("rows", index), cols=[1], dest=a.describe().as2d())
    taken = start - ctx.device_info()["hbm_free"]
    assert taken >= nbytes
    granule = 4096
    while granule < taken - nbytes:
        granule *= 2
    view = a.describe()  # a descriptor keeps the array, and so the block, alive
    del a
    assert start - ctx.device_info()["hbm_free"] == taken
    del view
    assert abs(ctx.device_info()["hbm_free"] - start) <= granule


# ---- torch -----------------------------------------------------------------------------------------------------------------
def test_torch_tensors_in_a_process_that_imports_torch_first():
    """out= torch tensors on a side stream and on torch's default stream, DeviceArray.torch() and the way back in, in a fresh
    child process: torch must be imported before libgdhip.so is loaded to see the GPU"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devexport_torch_child.py")
    run = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=170)
    out = run.stdout + run.stderr
    if "NO_TORCH" in run.stdout:
        pytest.skip("torch is not installed")
    assert run.returncode == 0 and "TORCH_EXPORT_OK 6" in run.stdout, out[-3000:]
