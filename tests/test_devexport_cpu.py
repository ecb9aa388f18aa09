"""CPU tests of device-array output (WeightedSamples.getDeviceSamples / getDeviceWeights, devarray.DeviceArray): how
``params``, ``rows``, ``dtype``, ``order`` and ``out=`` are resolved into Context.export_device calls, on a context double whose
``export_device`` writes through devarray.host_view into numpy memory.  The kernels are the GPU tier's (test_gpu_devexport.py)."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import devexport_cases as xc  # noqa: E402
import devinput_cases as dc  # noqa: E402
from fake_ctx import FakeContext  # noqa: E402
from test_colexpr_cpu import ExprContext  # noqa: E402  (FakeContext plus expr_eval, answered by the g++ build of colexpr.hpp)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))
import build_colexpr  # noqa: E402

from getdist_amd import devarray  # noqa: E402

NAMES = ["a", "b", "c", "d", "e"]
DTYPES = [np.float64, np.float32, np.float16, "bfloat16"]


class HostBlock:
    """the double of _lib.ExportBlock: host memory behind ``ptr``"""

    def __init__(self, nbytes):
        self.mem = np.full(max(int(nbytes), 1), 0xA5, dtype=np.uint8)
        self.ptr, self.device, self.nbytes = self.mem.ctypes.data, 0, int(nbytes)

    def fetch(self, out):
        ctypes.memmove(out.ctypes.data, self.ptr, out.nbytes)
        return out


class ExportContext(ExprContext):
    """fake_ctx.FakeContext (with expr_eval) plus export_block / export_device as numpy states them"""

    def export_block(self, nbytes):
        return HostBlock(nbytes)

    def export_device(self, rows=None, cols=None, dest=None, stream=None):
        kind = "all" if rows is None else rows[0]
        if kind == "all":
            ix = np.arange(self.N)
        elif kind == "range":
            ix = np.arange(rows[1], rows[2])
        elif kind == "mask":
            assert np.asarray(rows[1]).shape == (self.N,)
            ix = np.flatnonzero(rows[1])
        elif kind == "rows":
            ix = np.asarray(rows[1], dtype=np.int64)
            assert ix.size == 0 or (ix.min() >= 0 and ix.max() < self.N)
        else:
            assert kind == "nonzero"
            ix = np.flatnonzero(self.s[:, rows[1]] != 0)
        self.log.append(("export", kind, None if cols is None else list(cols), dest is not None, stream))
        if dest is None:
            return len(ix)
        values = self._w()[ix][:, None] if cols is None else self.s[ix][:, list(cols)]
        assert dest.ndim == 2 and dest.shape == values.shape and all(s >= 0 for s in dest.strides)
        if dest.dtype == devarray.GD_DT_BF16:
            as16 = devarray.DevArray(dest.ptr, dest.shape, dest.strides, devarray.GD_DT_F16)
            devarray.host_view(as16).view(np.uint16)[...] = xc.bf16_model(values)
        else:
            view = devarray.host_view(dest)
            with np.errstate(over="ignore"):
                view[...] = values.astype(view.dtype)
        return len(ix)


@pytest.fixture(scope="module")
def mc():
    from getdist_amd.mcsamples import MCSamples

    ExportContext.lib = build_colexpr.load()
    r = np.random.default_rng(12)
    X = r.standard_normal((300, 5)) * np.array([1.0, 3.0, 70.0, 1e-3, 1e5]) + np.array([0.0, 1.0, 70.0, 0.0, 0.0])
    w = r.integers(1, 5, 300).astype(float)
    ll = 0.5 * np.sum(r.standard_normal((300, 2)) ** 2, axis=1)
    return MCSamples(samples=X, weights=w, loglikes=ll, names=NAMES, _context_factory=ExportContext)


def bits(x):
    return x.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[x.dtype.itemsize])


def exports(mc):
    return [e for e in mc.ctx.log if e[0] == "export"]


# ---- params ----------------------------------------------------------------------------------------------------------------
def test_all_parameters_every_dtype_and_order(mc):
    for dtype in DTYPES:
        for order in "CF":
            got = mc.getDeviceSamples(dtype=dtype, order=order)
            assert isinstance(got, devarray.DeviceArray) and got.shape == (300, 5)
            assert got.strides == ((5, 1) if order == "C" else (1, 300))
            assert np.array_equal(bits(got.numpy()), xc.narrowed(mc.samples, dtype))


def test_names_indices_paraminfo_and_expressions(mc):
    p = mc.getDeviceParams()
    expr = p.a * np.sqrt(np.abs(p.c) / 0.3)
    got = mc.getDeviceSamples(["c", 0, mc.paramNames.names[3], expr, np.int64(1), "c"]).numpy()
    s = mc.samples
    want = np.column_stack([s[:, 2], s[:, 0], s[:, 3], s[:, 0] * np.sqrt(np.abs(s[:, 2]) / 0.3), s[:, 1], s[:, 2]])
    assert np.array_equal(got, want)
    with pytest.raises(Exception, match="unknown parameter"):
        mc.getDeviceSamples(["a", "nosuch"])


def test_single_item_is_one_dimensional(mc):
    p = mc.getDeviceParams()
    for item, want in (("b", mc.samples[:, 1]), (2, mc.samples[:, 2]), (p.a + p.b, mc.samples[:, 0] + mc.samples[:, 1])):
        got = mc.getDeviceSamples(item, dtype=np.float32)
        assert got.shape == (300,) and got.strides == (1,)
        assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert mc.getDeviceSamples(["b"]).shape == (300, 1)


def test_more_expressions_than_spare_slots_are_served_in_groups(mc):
    p = mc.getDeviceParams()
    s = mc.samples
    exprs = [p.a + float(k) for k in range(6)]
    del mc.ctx.log[:]
    got = mc.getDeviceSamples(["b"] + exprs + ["c"], rows=p.c > 70.0, dtype=np.float32).numpy()
    keep = s[:, 2] > 70.0
    want = np.column_stack([s[:, 1]] + [s[:, 0] + float(k) for k in range(6)] + [s[:, 2]])[keep]
    assert np.array_equal(got, want.astype(np.float32))
    # the mask takes one of the four spare slots: a count, then groups of at most three expressions
    calls = exports(mc)
    assert [c[3] for c in calls] == [False, True, True] and all(c[1] == "nonzero" for c in calls)
    assert [len(c[2]) for c in calls[1:]] == [4, 4]
    # an expression that reads the loglikes keeps their slot free: two expressions per group beside the mask
    del mc.ctx.log[:]
    from getdist_amd import colexpr

    got = mc.getDeviceSamples([p.a * 2.0, colexpr.loglikes + 1.0, p.b - 1.0], rows=p.c > 70.0).numpy()
    assert np.array_equal(got, np.column_stack([s[:, 0] * 2.0, mc.loglikes + 1.0, s[:, 1] - 1.0])[keep])
    assert [len(c[2]) for c in exports(mc)[1:]] == [2, 1]


# ---- rows ------------------------------------------------------------------------------------------------------------------
def test_rows_forms(mc):
    s = mc.samples
    mask = s[:, 0] > 0.2
    index = np.array([5, -1, 5, 299, 0, -300])
    p = mc.getDeviceParams()
    both = mask & (s[:, 2] < 100.0)
    # (rows=, the same selection as numpy indexes the host arrays by)
    for rows, index_by in ((slice(10, 50), None), (slice(None, -280), None), (slice(200, None), None), (slice(50, 10), None),
                           (mask, None), (index, None), (list(index), None), ([], slice(0, 0)), (np.zeros(300, bool), None),
                           ((p.a > 0.2) & (p.c < 100.0), both), (p.a > 1e9, slice(0, 0))):
        index_by = rows if index_by is None else index_by
        got = mc.getDeviceSamples(["a", "e", "c"], rows=rows)
        assert np.array_equal(got.numpy(), s[index_by][:, [0, 4, 2]])
        w = mc.getDeviceWeights(rows=rows, dtype=np.float32)
        assert np.array_equal(w.numpy(), mc.weights[index_by].astype(np.float32))


def test_rows_refused(mc):
    p = mc.getDeviceParams()
    for bad in (slice(0, 100, 2), slice(None, None, -1), np.zeros(299, bool), np.array([0.5, 1.0]), np.zeros((2, 2), int), "a", 3, p.a + 1.0):
        with pytest.raises(ValueError, match="slice with step 1|boolean expression"):
            mc.getDeviceSamples(rows=bad)
    with pytest.raises(IndexError):
        mc.getDeviceSamples(rows=[0, 300])
    with pytest.raises(ValueError, match="float64, float32, float16"):
        mc.getDeviceSamples(dtype=np.int32)
    with pytest.raises(ValueError, match="order"):
        mc.getDeviceSamples(order="K")


def test_weights(mc):
    from getdist_amd.mcsamples import MCSamples

    assert np.array_equal(mc.getDeviceWeights().numpy(), mc.weights)
    assert np.array_equal(bits(mc.getDeviceWeights(dtype="bfloat16").numpy()), xc.bf16_model(mc.weights))
    unit = MCSamples(samples=mc.samples[:40], names=NAMES, _context_factory=ExportContext)
    assert np.array_equal(unit.getDeviceWeights(rows=slice(3, 9), dtype=np.float16).numpy(), np.ones(6, np.float16))


# ---- out= ------------------------------------------------------------------------------------------------------------------
def test_out_shape_checks_come_before_any_call(mc):
    del mc.ctx.log[:]
    for shape, kw in (((300, 4), {}), ((299, 5), {}), ((300,), {}), ((300, 5, 1), {}), ((300, 1), dict(params="a")),
                      ((20, 5), dict(rows=slice(0, 21)))):
        with pytest.raises(ValueError, match="out= must have"):
            mc.getDeviceSamples(out=dc.DevBuf(np.zeros(shape)), **kw)
    with pytest.raises(ValueError, match="non-negative strides"):
        mc.getDeviceSamples(out=dc.DevBuf(np.zeros((300, 5))[::-1]))
    with pytest.raises(TypeError, match="device array"):
        mc.getDeviceSamples(out=np.zeros((300, 5)))
    assert exports(mc) == []
    with pytest.raises(ValueError, match="out= must have"):  # (the row count of an expression is the device's to say)
        mc.getDeviceSamples(rows=mc.getDeviceParams().a > 0.0, out=dc.DevBuf(np.zeros((300, 5))))
    assert [c[3] for c in exports(mc)] == [False]


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16])
def test_strided_out_views_are_written_in_place(mc, dtype):
    s = mc.samples
    back, wide = np.full((320, 12), -7.0, dtype=dtype), np.full((12, 320), -7.0, dtype=dtype)
    for back, view, kw, want in ((back, back[3:303, 2:7], {}, s), (back, back[5:305:1, 1:11:2], {}, s), (wide, wide[4:9, 10:310].T, {}, s),
                                 (back, back[10:40, 3], dict(params="d", rows=slice(100, 130)), s[100:130, 3]),
                                 (back, back[::2, 5][:100], dict(params="b", rows=slice(0, 100)), s[:100, 1])):
        back[...] = -7.0
        out = dc.DevBuf(view)
        assert mc.getDeviceSamples(out=out, **kw) is out
        with np.errstate(over="ignore"):
            assert np.array_equal(view, want.astype(dtype))
        # everything outside the view still holds the sentinel: the same view of a map of the block marks what is inside
        inside = np.zeros(back.shape, bool)
        offset = view.__array_interface__["data"][0] - back.__array_interface__["data"][0]
        np.lib.stride_tricks.as_strided(inside.reshape(-1)[offset // back.itemsize:], view.shape,
                                        tuple(st // back.itemsize for st in view.strides))[...] = True
        assert inside.sum() == view.size and np.all(back[~inside] == -7.0)


def test_out_of_another_element_type_decides_the_conversion(mc):
    out = dc.DevBuf(np.zeros((300, 2), np.float16))
    mc.getDeviceSamples(["a", "c"], dtype=np.float64, out=out)
    assert np.array_equal(out.host, mc.samples[:, [0, 2]].astype(np.float16))


def test_stream_defaults_to_the_one_out_announces(mc):
    class Stream:
        cuda_stream = 0x7F00

    for kw, want in ((dict(out=dc.DevBuf(np.zeros((300, 5)), stream=77)), 77), (dict(out=dc.DevBuf(np.zeros((300, 5)), stream=None)), None),
                     (dict(out=dc.DevBuf(np.zeros((300, 5)), stream=77), stream=Stream()), 0x7F00),
                     (dict(out=dc.DevBuf(np.zeros((300, 5)), stream=77), stream=0), devarray.STREAM_LEGACY), ({}, None)):
        del mc.ctx.log[:]
        mc.getDeviceSamples(**kw)
        assert [c[4] for c in exports(mc)] == [want]


# ---- the host mirror, the result object --------------------------------------------------------------------------------------
def test_the_host_mirror_of_a_device_built_set_is_not_created(mc):
    """a set whose samples exist on the (double's) device only keeps that state through every export"""
    from getdist_amd.mcsamples import MCSamples

    twin = MCSamples(samples=mc.samples.copy(), weights=mc.weights.copy(), names=NAMES, _context_factory=ExportContext)
    want = twin.samples.copy()
    twin.__dict__["_samples"], twin.__dict__["_samples_on_device"] = None, True
    twin.ctx.download_samples = lambda: pytest.fail("the host mirror was asked for")
    p = twin.getDeviceParams()
    got = twin.getDeviceSamples(["a", p.b * 2.0], rows=p.c > 70.0, dtype=np.float32).numpy()
    keep = want[:, 2] > 70.0
    assert np.array_equal(got, np.column_stack([want[:, 0], want[:, 1] * 2.0])[keep].astype(np.float32))
    assert np.array_equal(twin.getDeviceWeights(rows=[-1, 0]).numpy(), twin.weights[[-1, 0]])
    assert not twin._host_mirror_ready


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_interface_dictionary(mc, dtype, order):
    a = mc.getDeviceSamples(["a", "b", "c"], rows=slice(0, 7), dtype=dtype, order=order)
    size = {np.float64: 8, np.float32: 4, np.float16: 2, "bfloat16": 2}[dtype]
    cai = a.__cuda_array_interface__
    assert cai["version"] == 3 and cai["shape"] == (7, 3) and cai["data"] == (a.ptr, False) and cai["stream"] is None
    assert cai["typestr"] == {np.float64: "<f8", np.float32: "<f4", np.float16: "<f2", "bfloat16": "<i2"}[dtype]
    assert cai["strides"] == ((3 * size, size) if order == "C" else (size, 7 * size))
    assert a.nbytes == 21 * size and a.strides == ((3, 1) if order == "C" else (1, 7))
    assert a.dtype == ("bfloat16" if dtype == "bfloat16" else np.dtype(dtype))
    v = mc.getDeviceSamples("a", rows=slice(0, 7), dtype=dtype)
    assert v.__cuda_array_interface__["shape"] == (7,) and v.__cuda_array_interface__["strides"] == (size,)


def test_describe_round_trips(mc):
    a = mc.getDeviceSamples(["a", "b", "c"], dtype=np.float32, order="F")
    d = devarray.describe(a)
    assert isinstance(d, devarray.DevArray) and d.owner is a
    assert (d.ptr, d.shape, d.strides, d.dtype, d.device, d.stream) == (a.ptr, (300, 3), (1, 300), devarray.GD_DT_F32, 0, None)
    assert np.array_equal(devarray.host_view(d), mc.samples[:, :3].astype(np.float32))
    through = devarray.describe(dc.DevBuf(np.zeros((2, 2)), stream=5))  # (the interface route is as it was)
    assert through.stream == 5
    b = mc.getDeviceSamples("a", dtype="bfloat16")
    assert devarray.describe(b).dtype == devarray.GD_DT_BF16 and devarray.describe(b).shape == (300,)


def test_torch_needs_torch_to_be_imported_already(mc, monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", None)
    with pytest.raises(RuntimeError, match="import torch first"):
        mc.getDeviceSamples("a").torch()


def test_a_context_without_export_device_says_so(mc):
    from getdist_amd.mcsamples import MCSamples

    plain = MCSamples(samples=mc.samples[:50], names=NAMES, _context_factory=FakeContext)
    with pytest.raises(NotImplementedError, match="export_device"):
        plain.getDeviceSamples()
    with pytest.raises(NotImplementedError, match="export_device"):
        plain.getDeviceWeights()
