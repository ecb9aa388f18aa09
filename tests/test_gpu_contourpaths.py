"""
GPU tests of the contour paths (gd_contour_paths, getdist_amd/contourpaths.py): the device result equals the oracle of
tests/contourpath_cases.py bit for bit -- vertices as uint64 views, flags and loop offsets -- over the whole case table,
which covers both routes of the link tables (LDS up to 2560 crossed edges, global scratch above), as separate calls, as
one mixed batch and as single-grid calls; and end to end from samples.
"""

import numpy as np
import pytest

import contourpath_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from getdist_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


def density_of(case):
    from getdist_amd.densities import Density2D

    return Density2D(case["x"], case["y"], case["P"])


def check(paths, want, what):
    assert len(paths) == len(want)
    for k, raw in enumerate(want):
        cc.assert_raw_equal(paths.raw[k], raw, "%s level %d" % (what, k))


def test_every_case_equals_the_oracle(ctx):
    """One call per number of levels (a call has one nc), the grids of different sizes side by side."""
    from getdist_amd.contourpaths import contour_paths

    orc = cc.oracle_of_cases()
    routes = set()
    for nc in (1, 3, 8):
        group = [c for c in cc.cases() if len(c["levels"]) == nc]
        assert group
        got = contour_paths([density_of(c) for c in group], np.array([c["levels"] for c in group]), ctx=ctx)
        for c, p in zip(group, got):
            check(p, orc[c["name"]], c["name"])
            assert np.array_equal(p.levels, c["levels"])
            routes |= {len(raw[0]) > 2560 for raw in orc[c["name"]] if len(raw[0])}
    assert routes == {False, True}  # the table holds tasks on both sides of the LDS cap
    n_cap = {c["name"][:10]: len(orc[c["name"]][0][0]) for c in cc.cases() if c["name"].startswith("cap_")}
    assert n_cap == {"cap_lds_2x": 2560, "cap_global": 2562}


def test_mixed_batch_of_37_tasks(ctx):
    """37 (grid, level) tasks of different sizes in a single call: every level of the table as a grid of its own."""
    from getdist_amd.contourpaths import contour_paths

    orc = cc.oracle_of_cases()
    tasks = [(c, k) for c in cc.cases() for k in range(len(c["levels"]))]
    picked = tasks[1::2][:37]  # every other one: all sizes, the global-scratch route included
    assert len(picked) == 37 and len({c["P"].shape for c, _ in picked}) >= 6
    assert any(len(orc[c["name"]][k][0]) > 2560 for c, k in picked)
    got = contour_paths([density_of(c) for c, _ in picked], np.array([[c["levels"][k]] for c, k in picked]), ctx=ctx)
    for (c, k), p in zip(picked, got):
        cc.assert_raw_equal(p.raw[0], orc[c["name"]][k], "%s level %d" % (c["name"], k))


def test_single_grid_calls(ctx):
    """B = 1, through Density2D.getContourPaths, non-square grids among them."""
    orc = cc.oracle_of_cases()
    names = ("all_above_2x7_nc1", "peak_inside_9x4_nc3", "ring_33x20_nc3", "two_peaks_noise_33x20_nc8", "all_below_2x2_nc1")
    by_name = {c["name"]: c for c in cc.cases()}
    for name in names:
        c = by_name[name]
        assert c["P"].shape[0] != c["P"].shape[1] or name.startswith("all_below")
        check(density_of(c).getContourPaths(c["levels"], ctx=ctx), orc[name], name)
    d = density_of(by_name["ring_33x20_nc3"])
    d.contours = by_name["ring_33x20_nc3"]["levels"]
    check(d.getContourPaths(ctx=ctx), orc["ring_33x20_nc3"], "levels from .contours")


def test_non_finite_grid_raises(ctx):
    from getdist_amd.contourpaths import contour_paths
    from getdist_amd.densities import DensitiesError

    by_name = {c["name"]: c for c in cc.cases()}
    good = by_name["peak_inside_9x4_nc3"]
    for bad_value in (np.nan, np.inf):
        P = by_name["ring_33x20_nc3"]["P"].copy()
        P[7, 3] = bad_value
        bad = dict(by_name["ring_33x20_nc3"], P=P)
        with pytest.raises(DensitiesError):
            contour_paths([density_of(good), density_of(bad)], [0.3, 0.2, 0.1], ctx=ctx)
    check(contour_paths([density_of(good)], good["levels"], ctx=ctx)[0], cc.oracle_of_cases()[good["name"]], "after the error")


def test_argument_checks(ctx):
    from getdist_amd._lib import GdhipError
    from getdist_amd.contourpaths import contour_paths
    from getdist_amd.densities import DensitiesError, Density2D

    c = {k["name"]: k for k in cc.cases()}["peak_inside_9x4_nc3"]
    d = density_of(c)
    with pytest.raises(DensitiesError):
        contour_paths([d], ctx=ctx)  # no levels given and no .contours
    for levels in (np.zeros(0), np.linspace(0.1, 0.9, 9)):
        with pytest.raises(ValueError):
            contour_paths([d], levels, ctx=ctx)
    thin = Density2D.__new__(Density2D)
    thin.x, thin.y, thin.P, thin.contours = np.array([0.0, 1.0, 2.0]), np.array([0.5]), np.ones((1, 3)), None
    with pytest.raises(ValueError):
        contour_paths([thin], [0.5], ctx=ctx)
    # the native entry refuses the same before any launch
    dev = ctx.alloc(c["P"].nbytes)
    dev.from_host(c["P"])
    try:
        for ny, nx, levels in ((9, 4, np.zeros((1, 0))), (9, 4, np.linspace(0.1, 0.9, 9)[None, :]), (1, 36, np.array([[0.5]]))):
            with pytest.raises(GdhipError) as err:
                ctx.contour_paths(dev, [0], [ny], [nx], np.arange(float(nx)), [0], np.arange(float(ny)), [0], levels)
            assert err.value.code == -1
        with pytest.raises(GdhipError) as err:  # an axis offset that leaves the axis array
            ctx.contour_paths(dev, [0], [9], [4], np.arange(4.0), [1], np.arange(9.0), [0], np.array([[0.5]]))
        assert err.value.code == -1
    finally:
        dev.free()


def test_end_to_end_from_samples(zoo):
    """A bounded parameter, so open lines occur: levels, paths and areas of three pairs."""
    from getdist_amd.mcsamples import MCSamples

    fx = zoo["c1_bounded"]
    mc = MCSamples(samples=fx["samples"], weights=fx["weights"], names=fx["names"], ranges=fx["ranges"])
    pairs = [("a", "d"), ("b", "d"), ("a", "b")]
    got = mc.get2DContourPaths(pairs, fine_bins_2D=128)  # (the Python oracle walks every cell: a smaller grid keeps it quick)
    assert len(got) == 3
    open_lines = 0
    for p in got:
        assert p.density.contours is not None and np.array_equal(p.levels, p.density.contours)
        assert len(p.levels) == len(mc.contours) and p.density.P.shape == (p.y.size, p.x.size)
        assert p.density.P.base is not None  # (a view of the batch's block: it went up as it is)
        for k, lv in enumerate(p.levels):
            cc.assert_raw_equal(p.raw[k], cc.oracle_paths(p.density.P, p.x, p.y, lv), "pair level %d" % k)
            open_lines += sum(1 for ln in p.lines(k) if not np.array_equal(ln[0], ln[-1]))
        areas = [p.area(k) for k in np.argsort(p.levels)]
        assert all(a > b > 0 for a, b in zip(areas[:-1], areas[1:]))
    assert open_lines > 0
    assert len(mc.get2DContourPaths(pairs, num_plot_contours=1)[0]) == 1
