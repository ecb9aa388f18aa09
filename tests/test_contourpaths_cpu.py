"""
CPU tests of the contour paths: the oracle of tests/contourpath_cases.py (the statement the device is held to bit for bit in
test_gpu_contourpaths.py) against contourpy -- the committed golden tests/golden/contourpaths.npz, and live when contourpy is
installed -- and the ContourPaths container on oracle output.

Comparison with contourpy: equal numbers of open and closed lines and of vertices, every vertex equal after canonicalising
(closed lines rotated to their smallest vertex, lines sorted) within 4 ulp of max(|pa|, |pb|) of its edge -- both formulas
round three times; the largest difference measured when the golden was written was 6.7e-16, 1.0 ulp of the larger edge end
(stored in the golden as max_abs_diff / max_ulp_diff) -- and filled(level, inf) areas within 1e-14 of the domain area.
"""

import os

import numpy as np
import pytest

import contourpath_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contourpaths.npz")


def paths_of(case):
    from getdist_amd.contourpaths import ContourPaths

    return ContourPaths(case["x"], case["y"], case["levels"], cc.oracle_of_cases()[case["name"]])


def domain_area(case):
    return float((case["x"][-1] - case["x"][0]) * (case["y"][-1] - case["y"][0]))


def by_name(name):
    return {c["name"]: c for c in cc.cases()}[name]


def test_case_table_is_the_one_the_issue_lists():
    shapes = {c["P"].shape for c in cc.cases()}
    assert {(2, 2), (2, 7), (9, 4), (5, 5), (33, 20), (64, 64), (129, 129)} <= shapes
    assert {len(c["levels"]) for c in cc.cases()} == {1, 3, 8}
    for c in cc.cases():
        if len(c["levels"]) > 1 and not c["name"].startswith("checkerboard"):
            assert c["levels"][0] > c["P"].max() and c["levels"][-1] < c["P"].min()
    orc = cc.oracle_of_cases()
    assert len(orc["checkerboard_129x129_nc1"][0][0]) > 30000
    assert max(len(raw[2]) - 1 for raw in orc["two_peaks_noise_129x129_nc3"]) > 50  # many small loops


def test_oracle_agrees_with_golden():
    g = np.load(GOLDEN)
    cases = cc.golden_cases()
    assert [c["name"] for c in cases] == g["case_names"].tolist()
    assert [cc.case_crc(c) for c in cases] == g["case_crc"].tolist(), "the case table changed: run make_golden_contourpaths.py"
    assert str(g["contourpy_version"]) and float(g["max_ulp_diff"]) <= 2.0
    line_off, closed, xy = g["line_off"], g["line_closed"], g["xy"]
    t = 0
    for ci, c in enumerate(cases):
        mine = paths_of(c)
        for k in range(len(c["levels"])):
            assert (int(g["task_case"][t]), int(g["task_level"][t])) == (ci, k)
            ref = [(bool(closed[q]), xy[line_off[q]:line_off[q + 1]]) for q in range(g["task_line_off"][t], g["task_line_off"][t + 1])]
            cc.compare_lines(cc.canonical_lines(mine.lines(k)), ref, c, "%s level %d" % (c["name"], k))
            assert abs(mine.area(k) - float(g["area"][t])) <= 1e-14 * domain_area(c), (c["name"], k)
            t += 1
    assert t == len(g["area"])


def test_oracle_agrees_with_contourpy_live():
    pytest.importorskip("contourpy")
    for c in cc.cases():  # the 129 x 129 cases too
        mine = paths_of(c)
        for k, (lines, area) in enumerate(cc.contourpy_reference(c)):
            cc.compare_lines(cc.canonical_lines(mine.lines(k)), cc.canonical_lines(lines), c, "%s level %d" % (c["name"], k))
            assert abs(mine.area(k) - area) <= 1e-14 * domain_area(c), (c["name"], k)


def test_lines_split_at_flagged_vertices():
    c = by_name("peak_edge_64x64_nc3")
    p = paths_of(c)
    xy, flag, off = p.raw[1]
    assert len(off) == 2 and 0 < flag.sum() < len(flag)  # one loop, part of it along the domain edge
    lines = p.lines(1)
    assert len(lines) == 1 and len(lines[0]) == int((flag == 0).sum())
    assert not np.array_equal(lines[0][0], lines[0][-1])
    assert lines[0][0, 1] == c["y"][-1] and lines[0][-1, 1] == c["y"][-1]  # it starts and ends on the upper edge
    loop = np.roll(xy, -(int(np.flatnonzero(flag)[-1]) + 1), axis=0)
    assert np.array_equal(lines[0], loop[:len(lines[0])])  # in loop order
    # a loop inside the domain comes back closed, a grid entirely above has no line at all
    inner = paths_of(by_name("peak_inside_33x20_nc3"))
    (ln,) = inner.lines(1)
    assert np.array_equal(ln[0], ln[-1]) and len(ln) == len(inner.raw[1][0]) + 1
    assert inner.lines(0) == [] and inner.lines(2) == []
    # a ring: the hole is a second closed line
    assert [bool(np.array_equal(q[0], q[-1])) for q in paths_of(by_name("ring_33x20_nc3")).lines(1)] == [True, True]


def test_polygons_drop_repeated_points_and_orient():
    c = by_name("all_above_2x2_nc1")
    p = paths_of(c)
    assert len(p.raw[0][0]) == 8 and np.all(p.raw[0][1] == 1)  # every corner twice, all on the boundary
    (ring,) = p.polygons(0)
    x, y = c["x"], c["y"]
    assert sorted(map(tuple, ring.tolist())) == sorted([(x[0], y[0]), (x[1], y[0]), (x[1], y[1]), (x[0], y[1])])
    assert cc.polygon_area(ring) == pytest.approx(domain_area(c), rel=1e-15)
    outer, hole = paths_of(by_name("ring_33x20_nc3")).polygons(1)
    assert cc.polygon_area(outer) > 0 > cc.polygon_area(hole)  # counter-clockwise outside, clockwise hole
    assert paths_of(by_name("all_below_5x5_nc1")).polygons(0) == []


def test_area():
    for name in ("ring_64x64_nc3", "checkerboard_9x4_nc3", "two_peaks_noise_64x64_nc3", "eighths_33x20_nc1"):
        c = by_name(name)
        p = paths_of(c)
        for k in range(len(p)):
            xy, _, off = p.raw[k]
            want = sum(cc.polygon_area(xy[a:b]) for a, b in zip(off[:-1], off[1:]))
            assert p.area(k) == pytest.approx(want, rel=1e-12, abs=1e-15)
            assert p.area(k) == pytest.approx(sum(cc.polygon_area(r) for r in p.polygons(k)), rel=1e-12, abs=1e-15)
    c = by_name("peak_inside_64x64_nc8")
    areas = [paths_of(c).area(k) for k in range(8)]
    assert areas[0] == 0 and areas[-1] == pytest.approx(domain_area(c), rel=1e-14)
    assert all(a < b for a, b in zip(areas[:-1], areas[1:]))  # the levels fall


def test_to_path_codes():
    Path = pytest.importorskip("matplotlib.path").Path
    p = paths_of(by_name("ring_33x20_nc3"))
    filled = p.to_path(1)
    rings = p.polygons(1)
    assert len(filled.vertices) == sum(len(r) + 1 for r in rings)
    want = []
    for r in rings:
        want += [Path.MOVETO] + [Path.LINETO] * (len(r) - 1) + [Path.CLOSEPOLY]
    assert filled.codes.tolist() == want
    at = np.cumsum([0] + [len(r) + 1 for r in rings])
    for r, a, b in zip(rings, at[:-1], at[1:]):
        assert np.array_equal(filled.vertices[a:b - 1], r) and np.array_equal(filled.vertices[b - 1], r[0])
    # lines: closed ones end with CLOSEPOLY, open ones do not
    edge = paths_of(by_name("peak_edge_64x64_nc3")).to_path(1, filled=False)
    assert edge.codes[0] == Path.MOVETO and set(edge.codes[1:].tolist()) == {Path.LINETO}
    closed = p.to_path(1, filled=False)
    assert closed.codes.tolist().count(Path.CLOSEPOLY) == 2 and closed.codes.tolist().count(Path.MOVETO) == 2
    assert len(p.to_path(0).vertices) == 0


def test_levels_default_to_the_contours_of_the_density():
    from getdist_amd.contourpaths import contour_paths
    from getdist_amd.densities import DensitiesError, Density2D

    c = by_name("peak_inside_9x4_nc3")
    d = Density2D(c["x"], c["y"], c["P"])
    assert d.contours is None
    with pytest.raises(DensitiesError):
        contour_paths([d])
    with pytest.raises(DensitiesError):
        d.getContourPaths()
    for levels in (np.zeros(0), np.linspace(0.1, 0.9, 9), np.zeros((2, 3)), [np.nan]):
        with pytest.raises(ValueError):
            contour_paths([d], levels)
    assert contour_paths([]) == []


def test_exported_names():
    import getdist_amd

    assert getdist_amd.ContourPaths is getdist_amd.contourpaths.ContourPaths
    assert getdist_amd.contour_paths is getdist_amd.contourpaths.contour_paths
    assert hasattr(getdist_amd.MCSamples, "get2DContourPaths") and hasattr(getdist_amd.Density2D, "getContourPaths")
