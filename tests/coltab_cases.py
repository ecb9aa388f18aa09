"""Tables and query points shared by tests/test_coltab_cpu.py (the g++ build of csrc/colexpr.hpp) and tests/test_gpu_coltab.py
(the kernel): the look-up nodes of column expressions -- np.interp, Density1D.Prob, Density2D.Prob -- against numpy, this
package's host spline and scipy's RectBivariateSpline.ev, bit for bit.  Everything here is host data; a reference value
is computed by the caller from the SAME arrays the node was built from."""

import numpy as np

KNOT_COUNTS = (1, 2, 3, 4, 5, 257, 4097)  # SPLINE1 takes those >= 4
GRIDS = ((4, 4), (5, 9), (33, 47))  # (nx, ny) of the 2D densities
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])


def knots(n, seed):
    """n strictly increasing, irregularly spaced knots around zero (so that +-0.0 fall inside for n > 1)"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.uniform(0.05, 1.0, n))
    return x - x[n // 2] - (0.01 if n > 1 else 0.0)


def queries(kn, n_random=4099, seed=99):
    """The query values of one axis: the specials, every knot, its two neighbours in the doubles, then ``n_random`` random
    values reaching a quarter of the span beyond both ends.  (The edge cases come first: a prefix of this vector still has
    them.)"""
    kn = np.asarray(kn, dtype=np.float64)
    span = max(kn[-1] - kn[0], 1.0)
    rng = np.random.default_rng(seed + len(kn))
    return np.concatenate([SPECIALS, kn, np.nextafter(kn, -np.inf), np.nextafter(kn, np.inf),
                           rng.uniform(kn[0] - 0.25 * span, kn[-1] + 0.25 * span, n_random)])


def interp_tables():
    """name -> (xp, fp, left, right) for np.interp"""
    out = {}
    for n in KNOT_COUNTS:
        rng = np.random.default_rng(100 + n)
        out["n%d" % n] = (knots(n, n), rng.standard_normal(n), None, None)
    xp = knots(257, 7)
    fp = np.random.default_rng(8).standard_normal(257)
    out["left_right"] = (xp, fp, -7.5, np.nan)
    rep = knots(9, 3)
    rep[4] = rep[3]  # a repeated knot: numpy picks the last of the equal ones
    rep[7] = rep[6] = rep[5]
    out["repeated"] = (rep, np.arange(9.0) ** 2 - 3.0, None, 11.0)
    out["all_equal"] = (np.full(3, 0.5), np.array([1.0, 2.0, 3.0]), None, None)
    # non-finite values: the slope is inf - inf = NaN or +-inf, so numpy's rescue branch (retry from the right-hand knot,
    # then fp[j] when both ends are equal) is what decides the result
    out["constant_inf"] = (knots(5, 4), np.full(5, np.inf), None, None)
    out["mixed_inf"] = (knots(6, 5), np.array([np.inf, 0.0, 1.0, -np.inf, -np.inf, np.nan]), 0.25, None)
    out["huge"] = (knots(4, 6), np.array([1e308, -1e308, 1e308, 5e-324]), None, None)
    return out


def density1d(n, seed=0):
    """(Density1D on a regular grid of n points, its grid)"""
    from getdist_amd.densities import Density1D

    rng = np.random.default_rng(200 + n + seed)
    x = -0.37 + 0.013 * np.arange(n)
    P = np.exp(-0.5 * ((x - x[n // 2]) / (0.2 * (x[-1] - x[0]))) ** 2) * (1.0 + 0.1 * rng.standard_normal(n))
    return Density1D(x, P), x


def density2d(nx, ny, seed=0):
    """(Density2D with P[iy, ix] on regular axes of nx and ny points, x, y)"""
    from getdist_amd.densities import Density2D

    rng = np.random.default_rng(300 + 100 * nx + ny + seed)
    x = -0.21 + 0.07 * np.arange(nx)
    y = 1.3 + 0.11 * np.arange(ny)
    P = np.exp(-0.5 * (((x[None, :] - x[nx // 2]) / (0.3 * (x[-1] - x[0]))) ** 2 + ((y[:, None] - y[ny // 2]) / (0.3 * (y[-1] - y[0]))) ** 2))
    return Density2D(x, y, P * (1.0 + 0.1 * rng.standard_normal((ny, nx)))), x, y


def queries2d(x, y, n_random=4099):
    """(qx, qy) of equal length: the four corners, every pairing of the specials, every x edge case with a y that walks through
    the y edge cases and the other way round, then random pairs beyond both ends"""
    qx, qy = queries(x, n_random, 5), queries(y, n_random, 6)
    ex, ey = qx[:len(qx) - n_random], qy[:len(qy) - n_random]
    k = len(SPECIALS)
    px = [np.array([x[0], x[0], x[-1], x[-1]]), np.repeat(SPECIALS, k), ex, np.resize(ex, len(ey)), qx[len(ex):]]
    py = [np.array([y[0], y[-1], y[0], y[-1]]), np.tile(SPECIALS, k), np.resize(ey, len(ex)), ey, qy[len(ey):]]
    return np.concatenate(px), np.concatenate(py)


def rows(q, n):
    """``q`` cut or repeated to n rows"""
    return np.resize(q, n)


def same_bits(got, want, what):
    """equal uint64 views; NaNs are compared as NaN-ness only"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.dtype == bool:
        assert np.array_equal(got, want), what
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)), what


def shared_interp(xp, fp, left=None, right=None):
    """np.interp(., xp, fp) whose expression nodes all hold ONE table (np.interp makes a new one per call)"""
    from getdist_amd.colexpr import ColumnExpr, col, lookup

    table = np.interp(col(0), xp, fp, left=left, right=right).args[-1]
    return lambda x: lookup("INTERP", table, x) if isinstance(x, ColumnExpr) else np.interp(x, xp, fp, left=left, right=right)


def limit_tables():
    """the four tables of limits_program: bag of functions that take host vectors (numpy, scipy: the expected values) and
    column expressions (the look-up nodes) alike"""
    import types

    xp, fp, _, _ = interp_tables()["n257"]
    rp, rf, _, rr = interp_tables()["repeated"]
    d1, _ = density1d(257)
    d2, _, _ = density2d(5, 9)
    return types.SimpleNamespace(i1=shared_interp(xp, fp), i4=shared_interp(rp, rf, right=rr),
                                 s1=lambda x: d1.Prob(x, 1), s2=lambda x, y: d2.Prob(x, y), d1=d1, d2=d2)


def limits_program(p, T):
    """Four distinct tables, a stack 16 deep and 128 instructions, table ops mixed with the exact arithmetic ops: a right-nested
    chain of 16 leaves, seven of them look-ups (41 instructions), 43 more leaves folded on from the left, one negation."""
    leaves = [T.i1(p.a), p.b, T.s2(p.a, p.b), p.c, T.s1(p.c), p.d, T.i4(p.b), p.a] * 2
    out = leaves[-1]
    for k, x in enumerate(reversed(leaves[:-1])):
        out = x - out if k % 2 else x * out
    xs = [p.a, 0.5, p.b, p.c, 1.5, p.d, 0.25]
    for k in range(43):
        x = xs[k % len(xs)]
        out = (out + x, out * x, out - x, np.maximum(out, x))[k % 4]
    return -out


def mixed_program(p, T):
    """look-ups inside comparisons, where, clip and sqrt"""
    v = np.sqrt(abs(T.s2(p.b * 0.5, p.a + 1.0))) / (1.0 + T.i1(p.c) ** 2)
    return np.where((T.s1(p.d) > 0.0) & ~(p.a < T.i4(p.b)), np.clip(v, 0.01, 0.9), -v * T.i1(p.a - p.b))
