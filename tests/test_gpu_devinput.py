"""GPU tier of device-array input (gd_upload_device, gd_fetch_device_array, gd_download_samples): every case installs the
same values twice, from a device buffer and from numpy, and the resident columns, spare columns and weights must be
bit-equal (the conversions to fp64 are exact).  Shapes sit at the edges of the three kernel paths, not at the
workload's size.  Refusals use arguments that never reach a kernel."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_cases as cc  # noqa: E402
import devinput_cases as dc  # noqa: E402
import golden_util as gu  # noqa: E402
from test_gpu_compose import check_limits, device_rows  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_MOMENTS = 1e-12
TOL_GRID = 1e-6


@pytest.fixture(scope="module")
def ctxs():
    """(feeder: the second context the buffers are filled through, device-route context, host-route context)"""
    from getdist_amd._lib import Context

    three = Context(0), Context(0), Context(0)
    yield three
    for c in three:
        c.close()


def describe(a, feeder, stream=None):
    from getdist_amd import devarray

    buf = dc.DevBuf(a, feeder, stream=stream)
    return devarray.describe(buf)


def assert_same_resident(dev, host, spare=True):
    assert (dev.N, dev.n, dev.weighted) == (host.N, host.n, host.weighted)
    for j in range(host.n + (host.EXTRA_COLS if spare else 0)):  # the sample columns, then the zeroed spare columns
        assert np.array_equal(device_rows(dev, j), device_rows(host, j)), j
    if host.weighted:
        assert np.array_equal(device_rows(dev, -2), device_rows(host, -2))
        assert dev.weights_integral() == host.weights_integral()
        assert dev.weight_stats() == host.weight_stats()
    else:
        assert device_rows(dev, -2) is None


def check_upload(ctxs, a, weights=None, keep=None, stream=None, w_stream=None):
    """``a``: a numpy array or a list of them (chains); the same for ``weights``; ``stream`` / ``w_stream``: the producer
    stream code the buffers announce"""
    feeder, dev, host = ctxs
    chains = a if isinstance(a, list) else [a]
    wchains = None if weights is None else (weights if isinstance(weights, list) else [weights])
    parts = [describe(c, feeder, stream).as2d() for c in chains]
    wparts = None if wchains is None else [describe(w, feeder, w_stream) for w in wchains]
    assert dev.upload_device(parts, wparts, keep) is True
    full = np.vstack([np.asarray(c, dtype=np.float64).reshape(len(c), -1) for c in chains])
    host.upload(np.ascontiguousarray(full if keep is None else full[:, keep]),
                None if wchains is None else np.concatenate([np.asarray(w, dtype=np.float64) for w in wchains]))
    assert_same_resident(dev, host)
    assert np.array_equal(device_rows(dev, 0), (full if keep is None else full[:, keep])[:, 0])


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 33, 50, 65])
@pytest.mark.parametrize("N", [1, 31, 33, 512, 513, 1025])
def test_row_major_fp64(ctxs, N, n):
    check_upload(ctxs, dc.values(N, n))


@pytest.mark.parametrize("n", [1, 50])
@pytest.mark.parametrize("N", [1, 513])
def test_column_major_fp64(ctxs, N, n):
    check_upload(ctxs, np.asfortranarray(dc.values(N, n)))


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("order", ["C", "F"])
def test_narrow_element_types(ctxs, dtype, order):
    check_upload(ctxs, np.array(dc.values(513, 50, dtype), order=order))


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16])
@pytest.mark.parametrize("view", ["cols_1_51", "every_other_row", "rows_from_5", "transposed", "stride0_column", "stride0_rows"])
def test_views_of_a_block(ctxs, view, dtype):
    check_upload(ctxs, dc.views(dc.block(dtype))[view])


def test_kept_columns(ctxs):
    check_upload(ctxs, dc.values(513, 50), keep=[0, 3, 49, 7])
    check_upload(ctxs, np.asfortranarray(dc.values(513, 50)), keep=[1, 3, 49])
    check_upload(ctxs, dc.views(dc.block(np.float32))["cols_1_51"], keep=list(range(1, 50)))


CHAIN_ROWS = (7, 513, 64)  # destination offsets 7 and 520: odd, and across a tile


@pytest.mark.parametrize("weights", [None, np.float64, np.float32], ids=["unweighted", "w_f64", "w_f32"])
def test_three_chains(ctxs, weights):
    chains = [dc.values(r, 50) + k for k, r in enumerate(CHAIN_ROWS)]
    w = None
    if weights:
        w = [np.random.default_rng(k).gamma(2.0, 1.0, r).astype(weights) for k, r in enumerate(CHAIN_ROWS)]
    check_upload(ctxs, chains, w)
    check_upload(ctxs, [np.asfortranarray(c) for c in chains], w)


@pytest.mark.parametrize("kind", ["small_integers", "large_integers", "real"])
def test_weight_kinds(ctxs, kind):
    r = np.random.default_rng(5)
    w = {"small_integers": r.integers(0, 256, 1025).astype(float), "large_integers": r.integers(1, 2000, 1025).astype(float),
         "real": r.gamma(2.0, 1.0, 1025)}[kind]
    check_upload(ctxs, dc.values(1025, 6), w)
    assert ctxs[1].weights_integral() == (kind != "real")
    check_upload(ctxs, dc.values(1025, 6), w.astype(np.float32))  # (exact in fp32 for the integers; rounded first for the reals)


def bf16_case(feeder, rows, cols, seed=9):
    """((rows, cols) bf16 bit patterns on the device as a DevArray, the same values as float64): every finite bf16 value
    may occur, denormals included"""
    from getdist_amd import devarray

    r = np.random.default_rng(seed)
    bits = (r.integers(0, 0x7F80, (rows, cols)) | (r.integers(0, 2, (rows, cols)) << 15)).astype(np.uint16)
    want = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    buf = feeder.alloc(bits.nbytes)
    buf.from_host(bits)
    return devarray.DevArray(buf.ptr, (rows, cols), (cols, 1), devarray.GD_DT_BF16, owner=buf), want


@pytest.mark.parametrize("layout", ["row_major", "column_major", "cols_1_to_49", "every_third_row"])
def test_bf16(ctxs, layout):
    from getdist_amd import devarray

    feeder, dev, host = ctxs
    d, want = bf16_case(feeder, 513, 50)
    if layout == "column_major":  # the same buffer read as the transpose
        d, want = devarray.DevArray(d.ptr, (50, 513), (1, 50), d.dtype, owner=d.owner), want.T
    elif layout == "cols_1_to_49":  # 2-byte aligned base, row_stride > n
        d, want = devarray.DevArray(d.ptr + 2, (513, 48), (50, 1), d.dtype, owner=d.owner), want[:, 1:49]
    elif layout == "every_third_row":
        d, want = devarray.DevArray(d.ptr, (171, 50), (150, 1), d.dtype, owner=d.owner), want[::3]
    assert dev.upload_device([d]) is True
    host.upload(np.ascontiguousarray(want))
    assert_same_resident(dev, host)
    assert np.array_equal(dev.fetch_device_array(d), want)


@pytest.mark.parametrize("stream,w_stream", [(1, 1), (2, None), (1, 2)], ids=["legacy", "per_thread", "two_streams"])
def test_producer_streams(ctxs, stream, w_stream):
    """buffers that announce a producer stream: an event is recorded on it and the context's stream waits for it"""
    w = np.random.default_rng(1).gamma(2.0, 1.0, 513)
    check_upload(ctxs, dc.values(513, 50), w, stream=stream, w_stream=w_stream)
    feeder, dev, _ = ctxs
    x = dc.values(33, 5, np.float32)
    assert np.array_equal(dev.fetch_device_array(describe(x, feeder, stream)), x)


def test_fetch_device_array(ctxs):
    feeder, dev, _ = ctxs
    x = dc.block(np.float32)
    for name, v in dc.views(x).items():
        assert np.array_equal(dev.fetch_device_array(describe(v, feeder)), v.astype(np.float64)), name
    d = describe(x[5:, 1:51], feeder)
    assert np.array_equal(dev.fetch_device_array(d.row(-1)), x[-1:, 1:51]) and np.array_equal(dev.fetch_device_array(d.column(2)), x[5:, 3:4])
    assert np.array_equal(dev.fetch_device_array(describe(x[::-1, 3], feeder)), x[::-1, 3])  # negative stride, turned round


# ---- refusals: none of these can reach a kernel ---------------------------------------------------------------------------
def test_refusals_leave_the_previous_set_resident(ctxs):
    from getdist_amd._lib import GD_ERR_BADARG, GD_ERR_DECLINED, GdDevPart

    feeder, dev, _ = ctxs
    before = dc.values(33, 4)
    assert dev.upload_device([describe(before, feeder)])
    d = describe(dc.values(64, 5), feeder)
    d6 = describe(dc.values(64, 6), feeder)

    def call(parts, nparts=None, dtype=0):
        arr = (GdDevPart * max(len(parts), 1))()
        for st, (base, rows, cols, rs, cs) in zip(arr, parts):
            st.base, st.rows, st.cols, st.row_stride, st.col_stride = base, rows, cols, rs, cs
        return dev.lib.gd_upload_device(dev.h, arr, len(parts) if nparts is None else nparts, dtype, 0, None, 0, None, 0)

    good = (d.ptr, 64, 5, 5, 1)
    cases = [
        (call([good], nparts=0), GD_ERR_BADARG),
        (call([(None, 64, 5, 5, 1)]), GD_ERR_BADARG),
        (call([good], dtype=7), GD_ERR_BADARG),
        (call([(d.ptr, 64, 5, -5, 1)]), GD_ERR_DECLINED),
        (call([good, (d6.ptr, 64, 6, 6, 1)]), GD_ERR_BADARG),
        (call([(d.ptr, 0, 5, 5, 1)]), GD_ERR_BADARG),
    ]
    for k, (got, want) in enumerate(cases):
        assert got == want, k
        assert dev.lib.gd_last_error(dev.h)
    n64, nn = C.c_int64(), C.c_int64()
    dev._check(dev.lib.gd_num_rows(dev.h, C.byref(n64), C.byref(nn)))
    assert (n64.value, nn.value) == (33, 4)
    for j in range(4):
        assert np.array_equal(device_rows(dev, j), before[:, j])


# ---- the constructor -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feeder(ctxs):
    return ctxs[0]


def mc_pair(feeder, samples, weights=None, loglikes=None, **kw):
    from getdist_amd.mcsamples import MCSamples

    def wrap(v):
        if v is None:
            return None
        return [wrap(a) for a in v] if isinstance(v, list) else dc.DevBuf(v, feeder)

    dev = MCSamples(samples=wrap(samples), weights=wrap(weights), loglikes=wrap(loglikes), **kw)
    host = MCSamples(samples=samples, weights=weights, loglikes=loglikes, **kw)
    return dev, host


def assert_same_mcsamples(dev, host):
    assert (dev.numrows, dev.n) == (host.numrows, host.n)
    assert [p.name for p in dev.paramNames.names] == [p.name for p in host.paramNames.names]
    assert (dev.chain_offsets is None) == (host.chain_offsets is None)
    assert dev.chain_offsets is None or np.array_equal(dev.chain_offsets, host.chain_offsets)
    assert (dev.weights is None) == (host.weights is None) and (dev.weights is None or np.array_equal(dev.weights, host.weights))
    assert (dev.loglikes is None) == (host.loglikes is None) and (dev.loglikes is None or np.array_equal(dev.loglikes, host.loglikes))
    assert_same_resident(dev.ctx, host.ctx)


@pytest.mark.parametrize("ignore", [None, 3])
def test_constructor_three_chains(feeder, ignore):
    chains = [dc.values(r, 5) + np.random.default_rng(k).standard_normal((r, 5)) for k, r in enumerate(CHAIN_ROWS)]
    w = [np.random.default_rng(k).integers(1, 5, r).astype(float) for k, r in enumerate(CHAIN_ROWS)]
    w[1] = w[1].astype(np.float32)  # one chain's weights in fp32
    kw = {} if ignore is None else dict(settings=dict(ignore_rows=ignore))
    dev, host = mc_pair(feeder, chains, w, **kw)
    assert not dev._host_mirror_ready
    assert_same_mcsamples(dev, host)
    assert np.array_equal(dev.chain_offsets, np.cumsum([0] + [r - (ignore or 0) for r in CHAIN_ROWS]))
    dev.ctx.close(), host.ctx.close()


def test_constructor_drops_a_fixed_column(feeder):
    x = np.random.default_rng(8).standard_normal((257, 6))
    x[:, 2] = 0.25
    x[0, 4] = x[-1, 4]  # a candidate that does move
    names = list("abcdef")
    dev, host = mc_pair(feeder, x, names=names)
    assert not dev._host_mirror_ready and dev.n == 5 and "c" not in dev.index
    assert dev.ranges.lower["c"] == dev.ranges.upper["c"] == host.ranges.lower["c"] == 0.25
    assert_same_mcsamples(dev, host)
    dev.ctx.close(), host.ctx.close()


def test_constructor_statistics_densities_and_the_lazy_mirror(feeder):
    r = np.random.default_rng(21)
    g = r.standard_normal((1025, 6))
    x = g @ (np.eye(6) + 0.3 * np.tri(6, k=-1)) + np.arange(6)
    w, ll = r.gamma(2.0, 1.0, 1025), 0.5 * np.sum(g**2, axis=1)
    names = list("abcdef")
    dev, host = mc_pair(feeder, x, w, ll, names=names)
    assert_same_mcsamples(dev, host)
    assert gu.relerr(dev.getMeans(), host.getMeans()) < TOL_MOMENTS and gu.relerr(dev.cov(), host.cov()) < TOL_MOMENTS
    assert gu.relerr(dev.getVars(), host.getVars()) < TOL_MOMENTS and gu.relerr(dev.corr(), host.corr()) < TOL_MOMENTS
    dm, hm = dev.getMargeStats(), host.getMargeStats()
    for nm in names:
        want = hm.parWithName(nm)
        check_limits(dm.parWithName(nm), cc.limit_rows(want), [want.mean, want.err])
    d1, h1 = dev.get1DDensities(["a", "d"]), host.get1DDensities(["a", "d"])
    for a, b in zip(d1, h1):
        assert np.max(np.abs(a.P - b.P)) < TOL_GRID * np.max(b.P)
    d2, h2 = dev.get2DDensities([("a", "b")])[0], host.get2DDensities([("a", "b")])[0]
    assert np.max(np.abs(d2.P - h2.P)) < TOL_GRID * np.max(h2.P)
    dev.PCA(["a", "b", "c"])
    pd, ph = dev.getDeviceParams(), host.getDeviceParams()  # a column expression, evaluated over the resident columns
    assert dev.mean(pd.a * pd.b + 1.0, where=pd.c > 2.0) == host.mean(ph.a * ph.b + 1.0, where=ph.c > 2.0)
    ls_d, ls_h = dev.getLikeStats(), host.getLikeStats()  # (the best-fit sample: one row read from the device)
    assert [p.bestfit_sample for p in ls_d.names] == [p.bestfit_sample for p in ls_h.names]
    assert not dev._host_mirror_ready

    twin = dev.copy()
    assert not dev._host_mirror_ready and not twin._host_mirror_ready
    assert_same_resident(twin.ctx, dev.ctx, spare=False)  # (a clone does not take the spare columns over: the loglikes)

    got = dev.samples
    assert dev._host_mirror_ready and got.shape == (1025, 6) and np.array_equal(got, x)
    assert dev.samples is got and not twin._host_mirror_ready
    twin.ctx.close(), dev.ctx.close(), host.ctx.close()


def test_min_weight_ratio_takes_the_host_route(feeder):
    x = np.random.default_rng(2).standard_normal((300, 3))
    w = np.random.default_rng(3).gamma(2.0, 1.0, 300)
    w[17] = 1e-40
    dev, host = mc_pair(feeder, x, w)
    assert dev.numrows == host.numrows == 299 and dev._host_mirror_ready
    assert_same_mcsamples(dev, host)
    assert np.array_equal(dev.samples, host.samples)
    dev.ctx.close(), host.ctx.close()


def test_page_locked_memory_is_declined_to_the_host_route(feeder):
    """host-pinned memory behind the interface: gd_upload_device declines it with its own status and the constructor reads
    it from the host"""
    from getdist_amd.mcsamples import MCSamples

    x = feeder.pinned_array((300, 3))
    x[:] = np.random.default_rng(6).standard_normal((300, 3))

    class Pinned:
        __cuda_array_interface__ = dict(shape=x.shape, typestr="<f8", data=(x.ctypes.data, False), version=3, strides=None,
                                        stream=None)

    dev, host = MCSamples(samples=Pinned()), MCSamples(samples=np.array(x))
    assert dev._host_mirror_ready
    assert_same_mcsamples(dev, host)
    dev.ctx.close(), host.ctx.close()


def test_torch_tensors_in_a_process_that_imports_torch_first():
    """torch tensors (bf16 and fp32, produced on a side stream and on torch's default stream straight before the constructor
    call) in a fresh child process: torch must be imported before libgdhip.so is loaded to see the GPU, and
    this process has loaded the library long ago"""
    import subprocess

    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devinput_torch_child.py")
    run = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=170)
    out = run.stdout + run.stderr
    if "NO_TORCH" in run.stdout:
        pytest.skip("torch is not installed")
    assert run.returncode == 0 and "TORCH_CASES_OK 4" in run.stdout, out[-3000:]
