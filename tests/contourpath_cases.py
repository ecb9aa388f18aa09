"""Shared by test_contourpaths_cpu.py and test_gpu_contourpaths.py: the oracle of the contour-path semantics (the
straightforward per-cell loop: a dictionary of links, traced from the smallest edge id) and the seeded case table."""

import functools

import numpy as np


# ---- the oracle ------------------------------------------------------------------------------------------------------
def oracle_paths(P, x, y, level):
    """(xy[n, 2] float64, flag[n] uint8, loop_off[nloops + 1] int64) of the boundary of {P > level}: see gd_contour_paths in
    include/gdhip.h.  Plain Python floats: IEEE doubles, one rounding per operation."""
    ny, nx = P.shape
    z = [[float(v) for v in row] for row in P]
    xs, ys, L = [float(v) for v in x], [float(v) for v in y], float(level)
    NH = (ny + 2) * (nx + 1)

    def real(j, i):
        return 1 <= j <= ny and 1 <= i <= nx

    def above(j, i):
        return real(j, i) and z[j - 1][i - 1] > L

    def hid(j, i):
        return j * (nx + 1) + i

    def vid(j, i):
        return NH + j * (nx + 2) + i

    links = {}
    for j in range(ny + 1):
        for i in range(nx + 1):
            corners = [(j, i), (j, i + 1), (j + 1, i + 1), (j + 1, i)]
            a = [above(*c) for c in corners]
            if all(a) or not any(a):
                continue
            edges = [hid(j, i), vid(j, i + 1), hid(j + 1, i), vid(j, i)]
            starts = [k for k in range(4) if a[k] and not a[(k + 1) % 4]]
            ends = [k for k in range(4) if not a[k] and a[(k + 1) % 4]]
            if len(starts) == 2:
                centre = False
                if all(real(*c) for c in corners):
                    z0, z1, z2, z3 = (z[cj - 1][ci - 1] for cj, ci in corners)
                    centre = 0.25 * (z0 + z1 + z2 + z3) > L
                for k in starts:
                    links[edges[k]] = edges[(k + 1) % 4 if centre else (k - 1) % 4]
            else:
                links[edges[starts[0]]] = edges[ends[0]]

    def mix(pa, pb, za, zb):
        f = (L - za) / (zb - za)
        return pa * (1 - f) + pb * f

    def vertex(e):
        if e < NH:
            j, i = divmod(e, nx + 1)  # (j, i)-(j, i+1)
            if i == 0:
                return xs[0], ys[j - 1], 1
            if i == nx:
                return xs[nx - 1], ys[j - 1], 1
            return mix(xs[i - 1], xs[i], z[j - 1][i - 1], z[j - 1][i]), ys[j - 1], 0
        j, i = divmod(e - NH, nx + 2)  # (j, i)-(j+1, i)
        if j == 0:
            return xs[i - 1], ys[0], 1
        if j == ny:
            return xs[i - 1], ys[ny - 1], 1
        return xs[i - 1], mix(ys[j - 1], ys[j], z[j - 1][i - 1], z[j][i - 1]), 0

    assert sorted(links) == sorted(links.values())  # every crossed edge starts one segment and ends one
    xy, flag, loop_off, seen = [], [], [0], set()
    for e0 in sorted(links):
        if e0 in seen:
            continue
        e = e0
        while e not in seen:
            seen.add(e)
            vx, vy, f = vertex(e)
            xy.append((vx, vy))
            flag.append(f)
            e = links[e]
        assert e == e0
        loop_off.append(len(xy))
    return (np.array(xy, dtype=np.float64).reshape(-1, 2), np.array(flag, dtype=np.uint8),
            np.array(loop_off, dtype=np.int64))


# ---- the cases -------------------------------------------------------------------------------------------------------
def _axes(ny, nx, rng):
    """Increasing, unevenly spaced axes inside [-3, 4]."""
    def one(n, lo, hi):
        t = np.arange(n) + rng.uniform(-0.3, 0.3, n)
        t = (t - t[0]) / (t[-1] - t[0])
        return lo + (hi - lo) * t

    return one(nx, -3.0, 4.0), one(ny, -2.0, 3.5)


def _peak(x, y, cx, cy, s):
    """A peak of height 1 and width s at (cx, cy).  Sums, products, quotients and square roots only, here and in every
    other grid of the table: those are correctly rounded everywhere, so the table is the same on every machine and the
    committed golden file fits it."""
    return 1.0 / (1.0 + ((x[None, :] - cx) / s) ** 2 + ((y[:, None] - cy) / s) ** 2)


def _levels(P, nc, rng, by_rank=False):
    """nc levels; with more than one, the first lies above the maximum and the last below the minimum.  ``by_rank`` puts
    the others between grid values of given rank -- in the flat parts of a noisy grid, where the small loops are."""
    lo, hi = float(P.min()), float(P.max())
    if by_rank:
        ranked = np.sort(P.reshape(-1))
        at = (np.linspace(0.15, 0.85, max(nc - 2, 1))[::-1] * (ranked.size - 2)).astype(int)
        inner = 0.5 * (ranked[at] + ranked[at + 1])
    else:
        inner = np.sort(rng.uniform(lo + 0.004 * (hi - lo), lo + 0.7 * (hi - lo), max(nc - 2, 1)))[::-1]
    if nc == 1:
        return inner[:1] if by_rank else np.array([lo + 0.37 * (hi - lo)])
    return np.concatenate([[hi + 1.0], inner, [lo - 1.0]])


def _threshold_grid(nx, dent):
    """2 x nx, every other column above 0.5: 6 * ceil(nx / 2) crossed edges; ``dent`` lowers one node, two edges fewer."""
    P = np.zeros((2, nx))
    P[:, 0::2] = 1.0
    if dent:
        P[1, 400] = 0.0
    return P


@functools.lru_cache(maxsize=None)
def cases():
    """[dict(name, P, x, y, levels)], seeded."""
    rng = np.random.default_rng(20240917)
    out = []

    def add(name, shape, make, nc=None, levels=None, by_rank=False):
        ny, nx = shape
        x, y = _axes(ny, nx, rng)
        P = np.ascontiguousarray(make(x, y), dtype=np.float64)
        assert P.shape == shape
        lv = np.asarray(levels, dtype=np.float64) if levels is not None else _levels(P, nc, rng, by_rank)
        out.append(dict(name="%s_%dx%d_nc%d" % (name, ny, nx, len(lv)), P=P, x=x, y=y, levels=lv))

    for shape in ((2, 2), (5, 5)):
        add("all_below", shape, lambda x, y: _peak(x, y, 0.5, 0.5, 2.0), levels=[2.0])
    for shape in ((2, 2), (2, 7), (9, 4), (33, 20)):
        add("all_above", shape, lambda x, y: 1.0 + _peak(x, y, 0.5, 0.5, 2.0), levels=[0.5])
    for shape, nc in (((5, 5), 1), ((9, 4), 3), ((33, 20), 3), ((64, 64), 8)):
        add("peak_inside", shape, lambda x, y: _peak(x, y, 0.4, 0.6, 0.9), nc=nc)
    for shape, nc in (((2, 7), 1), ((33, 20), 3), ((64, 64), 3)):
        add("peak_edge", shape, lambda x, y: _peak(x, y, 0.3, 3.4, 1.0), nc=nc)
    for shape, nc in (((2, 2), 1), ((5, 5), 3), ((33, 20), 1), ((64, 64), 3)):
        add("peak_corner", shape, lambda x, y: _peak(x, y, -2.9, -1.9, 1.5), nc=nc)
    for shape, nc in (((9, 4), 1), ((33, 20), 3), ((64, 64), 3)):
        add("ring", shape, lambda x, y: 1.0 / (1.0 + ((np.sqrt((x[None, :] - 0.5) ** 2 + (y[:, None] - 0.7) ** 2) - 1.6) / 0.45) ** 2), nc=nc)

    def noisy(x, y):
        return 0.8 * _peak(x, y, -1.0, 0.0, 0.8) + 0.6 * _peak(x, y, 3.6, 2.0, 0.9) + 3e-3 * (rng.uniform(-1, 1, (3, y.size, x.size)).sum(axis=0))

    for shape, nc in (((5, 5), 1), ((33, 20), 8), ((64, 64), 3), ((129, 129), 3)):
        add("two_peaks_noise", shape, noisy, nc=nc, by_rank=True)

    def checker(x, y):
        return 1.0 - 2.0 * ((np.arange(y.size)[:, None] + np.arange(x.size)[None, :]) % 2)

    # the mean of an interior cell's corners is 0: above the level, below it, exactly at it
    for shape in ((2, 2), (5, 5), (9, 4), (64, 64)):
        add("checkerboard", shape, checker, levels=[-0.5, 0.5, 0.0])
    for shape in ((9, 4), (33, 20), (64, 64)):  # ties at nodes: a node exactly at the level is below
        add("eighths", shape, lambda x, y: np.round(8 * (_peak(x, y, 0.2, 0.4, 1.4) + 0.2 * _peak(x, y, 3.0, 3.0, 0.6))) / 8,
            levels=[0.5])
    add("checkerboard", (129, 129), checker, levels=[0.0])  # about 3e4 crossed edges: the global-scratch route
    # either side of the table cap of csrc/contourpaths.hip (CP_LDS_SLOTS = 2560 crossed edges)
    add("cap_lds", (2, 853), lambda x, y: _threshold_grid(853, True), levels=[0.5])
    add("cap_global", (2, 853), lambda x, y: _threshold_grid(853, False), levels=[0.5])
    return out


@functools.lru_cache(maxsize=None)
def oracle_of_cases():
    """{case name: [(xy, flag, loop_off) per level]}, computed once per process; the arrays are read-only."""
    res = {}
    for c in cases():
        per_level = [oracle_paths(c["P"], c["x"], c["y"], lv) for lv in c["levels"]]
        for raw in per_level:
            for a in raw:
                a.setflags(write=False)
        res[c["name"]] = per_level
    return res


def assert_raw_equal(got, want, what=""):
    """Bit for bit: xy as uint64 views, flag and loop_off."""
    gxy, gflag, goff = got
    wxy, wflag, woff = want
    assert np.array_equal(np.asarray(goff, dtype=np.int64), np.asarray(woff, dtype=np.int64)), "%s: loop offsets differ" % what
    assert np.array_equal(np.asarray(gflag, dtype=np.uint8), wflag), "%s: flags differ" % what
    g = np.ascontiguousarray(gxy, dtype=np.float64).reshape(-1, 2).view(np.uint64)
    w = np.ascontiguousarray(wxy, dtype=np.float64).reshape(-1, 2).view(np.uint64)
    assert g.shape == w.shape and np.array_equal(g, w), "%s: vertices differ" % what


# ---- comparison with a host contouring library -------------------------------------------------------------------------
def canonical_lines(lines):
    """Closed lines (first point repeated at the end) rotated to their lexicographically smallest vertex, then all lines
    sorted: [(closed, (m, 2) array without the repeated point)]."""
    out = []
    for ln in lines:
        ln = np.asarray(ln, dtype=np.float64).reshape(-1, 2)
        closed = len(ln) > 2 and bool(np.all(ln[0] == ln[-1]))
        if closed:
            ln = ln[:-1]
            k = min(range(len(ln)), key=lambda q: (ln[q, 0], ln[q, 1]))
            ln = np.roll(ln, -k, axis=0)
        out.append((closed, ln))
    out.sort(key=lambda t: (t[0], len(t[1]), t[1].ravel().tolist()))
    return out


def polygon_area(ring):
    """Signed area (shoelace) of a closed ring given without a repeated end point."""
    r = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    if len(r) < 3:
        return 0.0
    xn, yn = np.roll(r[:, 0], -1), np.roll(r[:, 1], -1)
    return 0.5 * float(np.sum(r[:, 0] * yn - xn * r[:, 1]))


def vertex_tolerance(v, axis):
    """4 ulp of max(|pa|, |pb|), pa and pb the axis values that bracket the coordinates ``v``: the oracle's formula and a
    host library's both round three times, under 2 ulp of the larger edge end together (measured: tests/golden)."""
    axis = np.asarray(axis, dtype=np.float64)
    i = np.clip(np.searchsorted(axis, v), 1, len(axis) - 1)
    return 4 * np.spacing(np.maximum(np.abs(axis[i - 1]), np.abs(axis[i])))


def compare_lines(mine, ref, case, what=""):
    """Counts (open and closed lines, vertices) equal and every vertex within vertex_tolerance, both sides canonical_lines.
    Returns the largest difference, absolute and in units of the tolerance's ulp."""
    assert [(c, len(p)) for c, p in mine] == [(c, len(p)) for c, p in ref], "%s: line or vertex counts differ" % what
    worst_abs = worst_ulp = 0.0
    for (_, p), (_, q) in zip(mine, ref):
        for col, axis in ((0, case["x"]), (1, case["y"])):
            d = np.abs(p[:, col] - q[:, col])
            tol = vertex_tolerance(q[:, col], axis)
            assert np.all(d <= tol), "%s: vertex off by %.3g (tolerance %.3g)" % (what, d.max(), tol[np.argmax(d)])
            if d.size:
                worst_abs, worst_ulp = max(worst_abs, float(d.max())), max(worst_ulp, float(np.max(d / (tol / 4))))
    return worst_abs, worst_ulp


def contourpy_reference(case):
    """[(lines, area of filled(level, inf))] per level from contourpy's serial algorithm."""
    import contourpy

    gen = contourpy.contour_generator(case["x"], case["y"], case["P"], name="serial", line_type=contourpy.LineType.Separate,
                                      fill_type=contourpy.FillType.OuterOffset)
    out = []
    for lv in case["levels"]:
        area = 0.0
        for pts, off in zip(*gen.filled(float(lv), np.inf)):
            for a, b in zip(off[:-1], off[1:]):
                area += polygon_area(pts[a:b - 1])  # (every ring repeats its first point)
        out.append((gen.lines(float(lv)), area))
    return out


def golden_cases():
    """The cases the golden file holds: sides up to 64."""
    return [c for c in cases() if max(c["P"].shape) <= 64]


def case_crc(case):
    import zlib

    return zlib.crc32(b"".join(np.ascontiguousarray(case[k], dtype=np.float64).tobytes() for k in ("P", "x", "y", "levels")))
