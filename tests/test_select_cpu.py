"""CPU tier of the device-side edits of a sample set: with a context double that has ``select_samples`` / ``set_weights``
(select_cases.FakeSelectContext) every mutator leaves the object the host route leaves -- the same call on a FakeContext
object --, without a host upload and without forming the host mirror."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import devinput_cases as dc  # noqa: E402
import select_cases as sc  # noqa: E402
from select_cases import FakeHostContext as FakeContext  # noqa: E402
from select_cases import FakeSelectContext  # noqa: E402
from test_devinput_cpu import FakeDevContext, assert_same_object  # noqa: E402

from getdist_amd._lib import GdhipError  # noqa: E402
from getdist_amd.mcsamples import MCSamples  # noqa: E402


@pytest.fixture(autouse=True)
def counters():
    FakeDevContext.device_uploads = FakeDevContext.host_uploads = FakeDevContext.downloads = 0
    FakeSelectContext.device_uploads = FakeSelectContext.host_uploads = FakeSelectContext.downloads = 0
    FakeSelectContext.selects = FakeSelectContext.weight_sets = 0


def pair(kind, source):
    inp = sc.inputs(kind)
    wrap = (lambda a: dc.DevBuf(np.ascontiguousarray(a))) if source == "device_arrays" else None
    dev = sc.make(MCSamples, inp, wrap, _context_factory=FakeSelectContext)
    host = sc.make(MCSamples, inp, _context_factory=FakeContext)
    assert dev._host_mirror_ready == (source == "host_arrays")
    return dev, host


@pytest.mark.parametrize("source", ["device_arrays", "host_arrays"])
@pytest.mark.parametrize("kind", ["single", "chains"])
@pytest.mark.parametrize("name", list(sc.MUTATORS))
def test_mutator_leaves_the_host_routes_object(name, kind, source):
    dev, host = pair(kind, source)
    uploads = FakeSelectContext.host_uploads
    apply, _, replaces_rows = sc.MUTATORS[name]
    apply(dev), apply(host)
    assert FakeSelectContext.host_uploads == uploads and FakeSelectContext.downloads == 0
    if replaces_rows:
        assert FakeSelectContext.selects >= 1 and not dev._host_mirror_ready
    else:  # the weights alone: the columns, and a mirror there is, stay
        assert (FakeSelectContext.selects, FakeSelectContext.weight_sets) == (0, 1)
        assert dev._host_mirror_ready == (source == "host_arrays")
    assert_same_object(dev, host)
    assert dev.needs_update == host.needs_update
    # ... and the numpy edit of the inputs, through a fresh object
    want = sc.expected(MCSamples, name, sc.inputs(kind), _context_factory=FakeContext)
    assert_same_object(dev, want)
    got = dev.samples  # the mirror, made on first read
    assert dev._host_mirror_ready and got.dtype == np.float64 and np.array_equal(got, host.samples)
    assert FakeSelectContext.downloads == (1 if replaces_rows or source == "device_arrays" else 0)


def test_setsamples_weight_filter_runs_on_the_device():
    inp = sc.inputs("single")
    w = inp["weights"] + 1.0
    w[[3, 77]] = 1e-40
    dev = MCSamples(samples=inp["samples"], names=list(sc.NAMES), _context_factory=FakeSelectContext)
    host = MCSamples(samples=inp["samples"], names=list(sc.NAMES), _context_factory=FakeContext)
    for mc in (dev, host):
        mc.setSamples(inp["samples"].copy(), w, inp["loglikes"])
    assert FakeSelectContext.selects == 1 and not dev._host_mirror_ready and dev.numrows == 1498
    assert_same_object(dev, host)
    assert np.array_equal(dev.samples, host.samples)


def test_float32_mirror_takes_the_host_route():
    inp = sc.inputs("single")
    objs = [MCSamples(samples=inp["samples"].astype(np.float32), weights=inp["weights"], names=list(sc.NAMES),
                      settings=dict(sc.SETTINGS), _context_factory=f) for f in (FakeSelectContext, FakeContext)]
    for mc in objs:
        mc.filter(inp["samples"][:, 0] > 0.1)
        mc.removeBurn(0.1)
    dev, host = objs
    assert FakeSelectContext.selects == 0 and dev._host_mirror_ready and dev.samples.dtype == np.float32
    assert_same_object(dev, host)
    assert np.array_equal(dev.samples, host.samples)


def snapshot(mc):
    return (mc.numrows, mc.n, [p.name for p in mc.paramNames.names], mc.weights.copy(), mc.loglikes.copy(), mc.ctx.s.copy(), mc.ctx.w.copy(),
            mc.means.copy(), mc._host_mirror_ready)


def same_snapshot(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("where", [np.ones(1499, dtype=bool), np.ones(1501, dtype=bool), np.array([0, 1500]), np.array([-1501])],
                         ids=["short_mask", "long_mask", "index_too_large", "index_too_negative"])
def test_selections_numpy_refuses_raise_numpys_error(where):
    dev, _ = pair("single", "host_arrays")
    before = snapshot(dev)
    with pytest.raises(IndexError):
        dev.filter(where)
    assert FakeSelectContext.selects == 0 and same_snapshot(snapshot(dev), before)


def test_no_rows_selected_raises_with_the_object_unchanged():
    for source in ("device_arrays", "host_arrays"):
        dev, _ = pair("single", source)
        before = snapshot(dev)
        with pytest.raises(GdhipError) as e:
            dev.filter(np.zeros(dev.numrows, dtype=bool))
        assert e.value.code == -1 and "no rows selected" in str(e.value)
        assert same_snapshot(snapshot(dev), before)


def test_negative_indices_count_from_the_end():
    dev, host = pair("single", "host_arrays")
    where = np.array([-1, 0, -1500, 7, 7])
    dev.filter(where), host.filter(where)
    assert FakeSelectContext.selects == 1
    assert_same_object(dev, host)


def test_remove_burn_fraction_equals_remove_burn():
    a, b = pair("chains", "device_arrays")[0], pair("chains", "device_arrays")[0]
    a.needs_update = b.needs_update = False
    a.removeBurnFraction(0.25), b.removeBurn(0.25)
    assert a.needs_update
    assert_same_object(a, b)


def test_doubles_without_the_calls_keep_the_host_route():
    dev = sc.make(MCSamples, sc.inputs("single"), lambda a: dc.DevBuf(np.ascontiguousarray(a)), _context_factory=FakeDevContext)
    assert not dev._host_mirror_ready
    dev.reweightAddingLogLikes(sc.EXTRA_LOGLIKES(dev.numrows))
    assert dev._host_mirror_ready and FakeDevContext.host_uploads == 1


def test_an_assigned_host_array_is_the_truth_until_it_is_uploaded():
    """``mc.samples = edited`` without setSamples: the next mutator works from that array, as it always did"""
    inp = sc.inputs("single")
    edited = inp["samples"].copy()
    edited[:, 1] = 0.25
    objs = [sc.make(MCSamples, inp, _context_factory=f) for f in (FakeSelectContext, FakeContext)]
    for mc in objs:
        mc.samples = edited
        assert mc.deleteFixedParams() == ([1], [0.25])
    assert FakeSelectContext.selects == 0
    assert_same_object(*objs)
    objs[0].removeBurn(0.1), objs[1].removeBurn(0.1)  # uploaded since: the device route again
    assert FakeSelectContext.selects == 1
    assert_same_object(*objs)
