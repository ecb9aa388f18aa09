"""The inputs and cases of tests/golden/raw_nd.npz (raw N-D densities): regenerated from seeds on any box, so the golden
file holds reference outputs only.  Shared by tests/golden/make_golden_nd.py and the CPU / GPU tests."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from getdist_amd import synth  # noqa: E402
from oracle.fixtures import _rng, loglikes_for, shapes_fixture  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raw_nd.npz")


def fixtures():
    """name -> (samples, weights, names, ranges, loglikes, weight kind)"""
    out = {}
    s, w, names, ranges = synth.config_c1(20_000)
    out["c1_unit"] = (s, w, names, ranges, loglikes_for(s), "unit")
    s, w, names, ranges = synth.config_c1(20_000, bounded=True)
    out["c1_bounded_unit"] = (s, w, names, ranges, loglikes_for(s, k=8), "unit")
    s, names, ranges = shapes_fixture()
    w = _rng(3).integers(1, 6, len(s)).astype(float)
    out["shapes_int"] = (s, w, names, ranges, loglikes_for(s, k=9), "int")
    s, w, names, ranges = synth.block_recipe(10, 20_000, weighted=True, stream=11)
    out["block10_real"] = (s, w, names, ranges, loglikes_for(s, k=10), "real")
    return out


# (parameters, kwargs, normalized): d = 1, 2, 3 at the default 12 bins, a 4D grid and a 2D grid with their own bin counts,
# one normalized=True grid (no contours / likes then), and one boundary_correction_order=0 case
CASES = {
    "c1_unit": [(["a"], {}, False), (["b", "a"], {}, False), (["a", "b", "c"], {}, False),
                (["a", "b", "c", "d"], {"num_bins_ND": 7}, False), (["c", "d"], {"num_bins_ND": 30}, False),
                (["a", "c"], {}, True)],
    "c1_bounded_unit": [(["d"], {}, False), (["a", "d"], {}, False), (["d", "c", "a"], {}, False),
                        (["d", "a", "b", "c"], {"num_bins_ND": 6}, False), (["d", "b"], {"num_bins_ND": 9}, False),
                        (["c", "d"], {}, True), (["d", "c"], {"boundary_correction_order": 0}, False)],
    "shapes_int": [(["s4"], {}, False), (["s4", "s5"], {}, False), (["s6", "s7", "s5"], {}, False),
                   (["s4", "s5", "s6", "s7"], {"num_bins_ND": 7}, False), (["s7", "s0"], {"num_bins_ND": 20}, False),
                   (["s5", "s6"], {}, True), (["s6", "s7"], {"boundary_correction_order": 0}, False)],
    "block10_real": [(["p5"], {}, False), (["p0", "p6"], {}, False), (["p5", "p6", "p7"], {}, False),
                     (["p4", "p5", "p8", "p9"], {"num_bins_ND": 7}, False), (["p1", "p7"], {"num_bins_ND": 25}, False),
                     (["p6", "p8"], {}, True)],
}


def case_key(fx, i):
    return "%s/%d" % (fx, i)


def case_spec(fx, i):
    pars, kw, normalized = CASES[fx][i]
    return json.dumps(dict(pars=pars, kw=kw, normalized=normalized), sort_keys=True)


def all_cases():
    for fx in CASES:
        for i in range(len(CASES[fx])):
            yield fx, i


def load_golden():
    return np.load(GOLDEN)


def pytest_approx(v):
    import pytest

    return pytest.approx(v, rel=1e-12, abs=0)


def make_samples(fx, **kw):
    """The fixture as a getdist_amd MCSamples (kw: e.g. _context_factory for the CPU double)."""
    from getdist_amd.mcsamples import MCSamples

    s, w, names, ranges, ll, _ = fixtures()[fx]
    return MCSamples(samples=s, weights=w, loglikes=ll, names=names, ranges=ranges, **kw)


def run_case(mc, fx, i):
    pars, kw, normalized = CASES[fx][i]
    if normalized:
        return mc.getRawNDDensity(pars, normalized=True, **kw)
    return mc.getRawNDDensityGridData(pars, meanlikes=True, maxlikes=True, **kw)


def check_case(d, gold, fx, i, exact):
    """Compare one computed DensityND with the golden.  exact: P and contours must be bit-equal (unit / integer weights,
    or any weights through the numpy double); otherwise P within 1e-10 of its max and contours to rtol 1e-9.  maxlikes
    and maxcontours are bit-equal in every case; likes within 1e-10 of its max."""
    key = case_key(fx, i)
    pars, kw, normalized = CASES[fx][i]
    assert str(gold[key + "/spec"]) == case_spec(fx, i), key
    P = gold[key + "/P"]
    assert d.P.shape == P.shape, key
    if exact:
        assert np.array_equal(d.P, P), key
    else:
        assert np.max(np.abs(d.P - P)) <= 1e-10 * np.max(np.abs(P)), key
    assert len(d.xs) == len(pars), key
    # axes and view ranges: bit-equal, or within the last-ulp differences of the parameter ranges that the 1D / 2D goldens
    # allow as well (the weighted range quantiles are summed in another order than the reference's; rtol 1e-13)
    for a, x in enumerate(d.xs):
        g = gold[key + "/x%d" % a]
        assert np.array_equal(x, g) or np.allclose(x, g, rtol=1e-13, atol=0), (key, a)
    vr, g = np.array(d.view_ranges, dtype=float), gold[key + "/view_ranges"]
    assert np.array_equal(vr, g) or np.allclose(vr, g, rtol=1e-13, atol=0), key
    assert d.spacing == pytest_approx(float(gold[key + "/spacing"])), key
    if normalized:
        return
    if exact:
        assert np.array_equal(d.contours, gold[key + "/contours"]), key
    else:
        np.testing.assert_allclose(d.contours, gold[key + "/contours"], rtol=1e-9, atol=0, err_msg=key)
    assert np.array_equal(d.maxlikes, gold[key + "/maxlikes"]), key
    assert np.array_equal(d.maxcontours, gold[key + "/maxcontours"]), key
    L = gold[key + "/likes"]
    assert np.max(np.abs(d.likes - L)) <= 1e-10 * np.max(np.abs(L)), key
