"""CPU tier of device-array input: devarray.describe on hand-made interface dicts, the span arithmetic, and the routing
of the MCSamples constructor, driven through a context double whose ``upload_device`` reads the described (host) memory
through ctypes.  The device-route object must equal the host-route object."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_cases as cc  # noqa: E402
import devinput_cases as dc  # noqa: E402
from fake_ctx import FakeContext  # noqa: E402

from getdist_amd import devarray  # noqa: E402
from getdist_amd.mcsamples import MCSamples, MCSamplesError  # noqa: E402


class Obj:
    def __init__(self, **cai):
        self.__cuda_array_interface__ = cai


# ---- describe ------------------------------------------------------------------------------------------------------------
def test_describe_v3_contiguous():
    d = devarray.describe(Obj(shape=(5, 3), typestr="<f8", data=(4096, False), version=3, strides=None, stream=None))
    assert (d.ptr, d.shape, d.strides, d.dtype, d.stream, d.device) == (4096, (5, 3), (3, 1), devarray.GD_DT_F64, None, None)


def test_describe_v2_has_no_stream_and_byte_strides_become_elements():
    d = devarray.describe(Obj(shape=(5, 3), typestr="<f4", data=(4100, False), version=2, strides=(208, 4)))
    assert (d.shape, d.strides, d.dtype, d.stream) == ((5, 3), (52, 1), devarray.GD_DT_F32, None)
    d = devarray.describe(Obj(shape=(7,), typestr="<f2", data=(64, True), version=3, strides=(6,), stream=None))
    assert (d.strides, d.dtype, d.as2d().shape, d.as2d().strides) == ((3,), devarray.GD_DT_F16, (7, 1), (3, 1))


@pytest.mark.parametrize("code,want", [(None, None), (1, devarray.STREAM_LEGACY), (2, devarray.STREAM_PER_THREAD),
                                       (0x7F00DEAD0000, 0x7F00DEAD0000), (0, devarray.STREAM_LEGACY)])
def test_describe_stream_codes(code, want):
    d = devarray.describe(Obj(shape=(2, 2), typestr="<f8", data=(4096, False), version=3, strides=None, stream=code))
    assert d.stream == want


@pytest.mark.parametrize("typestr", ["<i4", "<i8", "<u2", "<c16", "|b1", ">f8"])
def test_describe_rejects_other_element_types(typestr):
    with pytest.raises(TypeError) as e:
        devarray.describe(Obj(shape=(2, 2), typestr=typestr, data=(4096, False), version=3, strides=None))
    assert typestr in str(e.value) and "float64" in str(e.value)


def test_describe_rejects_old_versions_and_split_elements():
    with pytest.raises(TypeError):
        devarray.describe(Obj(shape=(2,), typestr="<f8", data=(4096, False), version=1))
    with pytest.raises(TypeError):
        devarray.describe(Obj(shape=(2, 2), typestr="<f8", data=(4096, False), version=3, strides=(12, 8)))


def test_host_objects_are_not_device_arrays():
    assert devarray.describe(np.zeros((3, 2))) is None
    assert devarray.describe([[1.0, 2.0]]) is None and devarray.describe(None) is None
    try:
        import torch
    except ImportError:
        return
    assert devarray.describe(torch.zeros(3, 2, dtype=torch.float64)) is None
    s = MCSamples(samples=torch.arange(12, dtype=torch.float64).reshape(6, 2) ** 2, _context_factory=FakeContext)
    assert s._host_mirror_ready and s.numrows == 6  # through np.asarray, as before


def test_describe_torch_tensor_by_attributes():
    """a tensor on the GPU is recognised by its attributes; the stream comes from the module its type came from"""
    import types

    fake = types.SimpleNamespace(cuda=types.SimpleNamespace(current_stream=lambda dev: types.SimpleNamespace(cuda_stream=fake.handle),
                                                            current_device=lambda: 0), handle=0x5000)
    sys.modules["faketorch"] = fake

    class Tensor:
        __module__ = "faketorch.tensor"
        is_cuda = True
        shape = (9, 4)

        def __init__(self, dtype):
            self.dtype, self.device = dtype, types.SimpleNamespace(index=None)

        def detach(self):
            return self

        def data_ptr(self):
            return 1 << 21

        def stride(self):
            return (8, 2)

    try:
        d = devarray.describe(Tensor("torch.bfloat16"))
        assert (d.ptr, d.shape, d.strides, d.dtype, d.device, d.stream) == (1 << 21, (9, 4), (8, 2), devarray.GD_DT_BF16, 0, 0x5000)
        fake.handle = 0  # torch's default stream is the legacy default stream: ordering IS needed
        assert devarray.describe(Tensor("torch.float32")).stream == devarray.STREAM_LEGACY
        with pytest.raises(TypeError) as e:
            devarray.describe(Tensor("torch.int64"))
        assert "torch.int64" in str(e.value) and "float64" in str(e.value)
    finally:
        del sys.modules["faketorch"]


# ---- span ----------------------------------------------------------------------------------------------------------------
def D(shape, strides, dtype=devarray.GD_DT_F64, ptr=1 << 20):
    return devarray.DevArray(ptr, shape, strides, dtype)


def test_span_arithmetic():
    assert D((5, 3), (3, 1)).span() == (0, 15 * 8)                      # contiguous
    assert D((5, 3), (52, 1), devarray.GD_DT_F32).span() == (0, (4 * 52 + 3) * 4)  # sliced columns
    assert D((300, 52), (104, 1)).span() == (0, (299 * 104 + 52) * 8)   # every other row
    assert D((600, 52), (52, 0)).span() == (0, (599 * 52 + 1) * 8)      # stride-0 column
    assert D((40, 52), (0, 1)).span() == (0, 52 * 8)                    # stride-0 rows
    assert D((1, 50), (999, 1)).span() == (0, 50 * 8)                   # one row: its stride reaches nothing
    assert D((4,), (-2,), devarray.GD_DT_F16).span() == (-12, 2)        # negative stride
    assert D((0, 5), (5, 1)).span() == (0, 0)
    x = dc.block()
    for name, v in dc.views(x).items():
        d = devarray.describe(dc.DevBuf(v))
        assert d.span() == dc.byte_span(v), name
        assert np.array_equal(devarray.host_view(d), v), name


def test_row_column_and_forward_views():
    x = dc.block()
    d = devarray.describe(dc.DevBuf(x[5:, 1:51]))
    assert np.array_equal(devarray.host_view(d.row(-1)), x[-1:, 1:51])
    assert np.array_equal(devarray.host_view(d.column(3)), x[5:, 4:5])
    assert np.array_equal(devarray.host_view(d.rows_from(590)), x[595:, 1:51])
    back = devarray.describe(dc.DevBuf(x[::-1, ::2]))
    fwd, flipped = back.forward()
    assert flipped == [0] and min(fwd.strides) > 0 and np.array_equal(devarray.host_view(fwd)[::-1], x[::-1, ::2])


# ---- the constructor's routing ------------------------------------------------------------------------------------------
class HostBlock:
    def __init__(self, nbytes):
        self.a = np.zeros(nbytes, dtype=np.uint8)
        self.ptr, self.nbytes = self.a.ctypes.data, nbytes

    def from_host(self, arr, offset_bytes=0):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.a[offset_bytes:offset_bytes + raw.size] = raw

    def free(self):
        pass


class FakeDevContext(FakeContext):
    """FakeContext with the device-input calls: the 'device' memory is host memory, read through ctypes."""

    device_uploads = host_uploads = downloads = fetched_values = 0

    def alloc(self, nbytes):
        return HostBlock(nbytes)

    def upload(self, samples, weights=None):
        type(self).host_uploads += 1
        super().upload(samples, weights)

    def fetch_device_array(self, desc):
        type(self).fetched_values += int(np.prod(desc.shape))
        return np.array(devarray.host_view(desc), dtype=np.float64)

    def upload_device(self, parts, weights=None, keep=None):
        if any(s < 0 for d in list(parts) + list(weights or []) for s in d.strides):
            return False  # gd_upload_device declines negative strides
        keep = list(range(parts[0].shape[1])) if keep is None else list(keep)
        s = np.vstack([np.array(devarray.host_view(p), dtype=np.float64)[:, keep] for p in parts])
        w = None if weights is None else np.concatenate([np.array(devarray.host_view(d), dtype=np.float64) for d in weights])
        FakeContext.upload(self, s, w)
        type(self).device_uploads += 1
        return True

    def download_samples(self):
        type(self).downloads += 1
        return self.s[:, :self.n].copy()

    def read_row(self, i):
        return self.s[i, :self.n].copy()

    def clone_samples(self, src):
        FakeContext.upload(self, src.s[:, :src.n], src.w)


@pytest.fixture(autouse=True)
def counters():
    FakeDevContext.device_uploads = FakeDevContext.host_uploads = FakeDevContext.downloads = FakeDevContext.fetched_values = 0


def wrap(v, dtype=None):
    """the fixture value (array, list of arrays, None) as device buffers"""
    if v is None:
        return None
    if isinstance(v, list):
        return [wrap(a, dtype) for a in v]
    return dc.DevBuf(np.ascontiguousarray(v, dtype=dtype))


def pair(fx, device_weights=True, **kw):
    """(device-route object, host-route object) of the fixture"""
    f = cc.fixtures()[fx]
    common = dict(names=list(f["names"]), ranges=dict(f["ranges"]), **kw)
    host = MCSamples(samples=f["samples"], weights=f["weights"], loglikes=f["loglikes"], _context_factory=FakeContext, **common)
    dev = MCSamples(samples=wrap(f["samples"]), weights=wrap(f["weights"]) if device_weights else f["weights"],
                    loglikes=wrap(f["loglikes"]) if device_weights else f["loglikes"], _context_factory=FakeDevContext, **common)
    return dev, host


def same_vector(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and np.array_equal(a, b))


def assert_same_object(dev, host):
    assert (dev.numrows, dev.n) == (host.numrows, host.n)
    assert [p.name for p in dev.paramNames.names] == [p.name for p in host.paramNames.names]
    assert (dev.ranges.lower, dev.ranges.upper) == (host.ranges.lower, host.ranges.upper)
    assert (dev.chain_offsets is None) == (host.chain_offsets is None)
    assert dev.chain_offsets is None or np.array_equal(dev.chain_offsets, host.chain_offsets)
    assert same_vector(dev.weights, host.weights) and same_vector(dev.loglikes, host.loglikes)
    assert np.array_equal(dev.ctx.s, host.ctx.s)
    assert (dev.ctx.w is None and host.ctx.w is None) or np.array_equal(dev.ctx.w, host.ctx.w)
    assert np.array_equal(dev.means, host.means) and np.array_equal(dev.fullcov, host.fullcov)


@pytest.mark.parametrize("ignore", [None, 3, 0.2], ids=["all_rows", "ignore_3", "ignore_20pct"])
@pytest.mark.parametrize("fx", ["A", "U", "MC", "ONE", "FXA"])
def test_device_route_gives_the_host_routes_object(fx, ignore):
    kw = {} if ignore is None else dict(settings=dict(ignore_rows=ignore))
    dev, host = pair(fx, **kw)
    assert (FakeDevContext.device_uploads, FakeDevContext.host_uploads) == (1, 0)
    assert not dev._host_mirror_ready and host._host_mirror_ready
    assert_same_object(dev, host)
    if fx == "FXA":  # the constant column is a zero-width range, left out through the kept-column list
        assert "c" not in dev.index and dev.ranges.lower["c"] == dev.ranges.upper["c"] == cc.FIXED_VALUE
    # only the probe rows, the candidate columns, the weights and the loglikes came to the host
    f = cc.fixtures()[fx]
    rows = sum(len(c) for c in f["samples"]) if isinstance(f["samples"], list) else len(f["samples"])
    vectors = (f["weights"] is not None) + (f["loglikes"] is not None) + (fx == "FXA")
    assert FakeDevContext.fetched_values <= vectors * rows + 2 * 5


def test_host_weights_with_device_samples():
    dev, host = pair("A", device_weights=False)
    assert FakeDevContext.device_uploads == 1 and not dev._host_mirror_ready
    assert_same_object(dev, host)
    dev, host = pair("MC", device_weights=False)
    assert_same_object(dev, host)


def test_one_dimensional_device_samples():
    x = np.random.default_rng(3).standard_normal(41)
    dev = MCSamples(samples=dc.DevBuf(x), names=["x"], _context_factory=FakeDevContext)
    host = MCSamples(samples=x, names=["x"], _context_factory=FakeContext)
    assert FakeDevContext.device_uploads == 1
    assert_same_object(dev, host)


def test_min_weight_ratio_that_removes_rows_takes_the_host_route():
    f = cc.fixtures()["A"]
    w = f["weights"].copy()
    w[17] = 1e-40 * w.max()  # one entry below min_weight_ratio (1e-30) x the maximum
    kw = dict(names=list(f["names"]), loglikes=f["loglikes"])
    host = MCSamples(samples=f["samples"], weights=w, _context_factory=FakeContext, **kw)
    dev = MCSamples(samples=dc.DevBuf(np.ascontiguousarray(f["samples"])), weights=dc.DevBuf(w), _context_factory=FakeDevContext,
                    **kw)
    assert (FakeDevContext.device_uploads, FakeDevContext.host_uploads) == (0, 1)
    assert dev.numrows == host.numrows == len(w) - 1 and dev._host_mirror_ready
    assert_same_object(dev, host)
    assert np.array_equal(dev.samples, host.samples)


def test_negative_strides_are_declined_to_the_host_route():
    f = cc.fixtures()["U"]
    x = np.ascontiguousarray(f["samples"])
    dev = MCSamples(samples=dc.DevBuf(x[::-1]), names=list(f["names"]), _context_factory=FakeDevContext)
    host = MCSamples(samples=x[::-1], names=list(f["names"]), _context_factory=FakeContext)
    assert (FakeDevContext.device_uploads, FakeDevContext.host_uploads) == (0, 1)
    assert_same_object(dev, host)


class DecliningContext(FakeDevContext):
    """a context whose device calls decline everything, as the library does for memory the host can read as well"""

    kind = 1  # GD_PTR_PINNED

    def upload_device(self, parts, weights=None, keep=None):
        return False

    def fetch_device_array(self, desc):
        return None

    def pointer_info(self, ptr):
        return type(self).kind, -1


def test_declined_memory_is_read_from_the_host_only_where_the_host_can():
    f = cc.fixtures()["A"]
    kw = dict(names=list(f["names"]), loglikes=f["loglikes"])
    host = MCSamples(samples=f["samples"], weights=f["weights"], _context_factory=FakeContext, **kw)
    x = np.ascontiguousarray(f["samples"])
    DecliningContext.kind = 1
    dev = MCSamples(samples=dc.DevBuf(x), weights=dc.DevBuf(f["weights"]), _context_factory=DecliningContext, **kw)
    assert dev._host_mirror_ready
    assert_same_object(dev, host)
    DecliningContext.kind = 3  # GD_PTR_UNKNOWN: never dereferenced from the host
    with pytest.raises(MCSamplesError):
        MCSamples(samples=dc.DevBuf(x), _context_factory=DecliningContext, names=list(f["names"]))
    DecliningContext.kind = 1


def test_a_list_of_device_vectors_is_refused_clearly():
    with pytest.raises(TypeError) as e:
        MCSamples(samples=[dc.DevBuf(np.arange(5.0)), dc.DevBuf(np.arange(5.0) ** 2)], _context_factory=FakeDevContext)
    assert "stack" in str(e.value)


def test_mirror_is_made_on_first_read_and_kept():
    dev, host = pair("A")
    assert not dev._host_mirror_ready
    assert np.array_equal(dev.getMeans(), host.getMeans()) and np.array_equal(dev.getVars(), host.getVars())
    assert np.array_equal(dev.cov(), host.cov()) and np.array_equal(dev.corr(), host.corr())
    twin = dev.copy()
    assert not dev._host_mirror_ready and not twin._host_mirror_ready and FakeDevContext.downloads == 0
    assert np.array_equal(twin.ctx.s, dev.ctx.s)
    got = dev.samples
    assert dev._host_mirror_ready and FakeDevContext.downloads == 1
    assert got.shape == host.samples.shape and np.array_equal(got, host.samples)
    assert dev.samples is got and FakeDevContext.downloads == 1
    assert not twin._host_mirror_ready
    # a mutator that rebuilds the set on the host works from then on as it does for a host-built set
    dev.removeBurn(0.1), host.removeBurn(0.1)
    assert_same_object(dev, host)
    twin.filter(np.arange(0, twin.numrows, 2))
    assert twin._host_mirror_ready


def test_column_share_refuses_device_arrays():
    with pytest.raises(MCSamplesError):
        MCSamples(samples=dc.DevBuf(np.zeros((4, 2))), column_share=object(), _context_factory=FakeDevContext)


def test_device_must_match():
    d = devarray.describe(dc.DevBuf(dc.values(9, 2)))
    d.device = 1
    with pytest.raises(ValueError) as e:
        MCSamples(samples=d, _context_factory=FakeDevContext)
    assert "device=1" in str(e.value)
