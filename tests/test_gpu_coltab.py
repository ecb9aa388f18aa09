"""GPU tier of the table look-ups of column expressions (gd_expr_eval_tab: np.interp, Density1D.Prob and Density2D.Prob of a
ColumnExpr): the kernel against np.interp, this package's Density1D.Prob of the host vector and scipy's
RectBivariateSpline.ev BIT FOR BIT (uint64 views; NaNs compared as NaN-ness) on the tables and query points of
coltab_cases.py, the four destinations, programs at the limits, the tallies, the argument checks, the unchanged table-free
path, and the look-ups end to end on an MCSamples.

np.log in a composite is the device library's, which numpy's differs from in the last bits (tests/test_gpu_colexpr.py bounds it
by 3 ulp): where a host route goes through np.log the comparison says so."""

import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coltab_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
N_ROWS = 20_011  # not a multiple of 64, 256 or 512
ROW_COUNTS = (1, 63, 513, N_ROWS)
PD = ctypes.POINTER(ctypes.c_double)
same_bits = cases.same_bits


class Bare:
    """What ColumnExpr needs of a sample set, over a bare Context: columns are addressed by index, or a, b, c, d = 0 .. 3"""

    loglikes = None

    def __init__(self, ctx):
        self.ctx, self.n = ctx, ctx.n

    def _col(self, par):
        return "abcd".index(par) if isinstance(par, str) else int(par)


def _upload(columns, weights=None):
    from getdist_amd._lib import Context

    X = np.asfortranarray(np.column_stack(columns))
    ctx = Context(0)
    ctx.upload(X, weights)
    return ctx, X


def _all_cases():
    """[(name, number of operands, function of host vectors and of expressions alike, query vector(s))]"""
    out = []
    for name, (xp, fp, left, right) in sorted(cases.interp_tables().items()):
        out.append(("interp " + name, lambda x, a=(xp, fp, left, right): np.interp(x, a[0], a[1], left=a[2], right=a[3]),
                    [cases.queries(xp)]))
    for n in cases.KNOT_COUNTS:
        if n >= 4:
            d1, x = cases.density1d(n)
            for d in ((0, 1, 2, 3) if n in (5, 4097) else (0,)):
                out.append(("spline1 n%d d%d" % (n, d), lambda x, d1=d1, d=d: d1.Prob(x, d), [cases.queries(x)]))
    for nx, ny in cases.GRIDS:
        d2, x, y = cases.density2d(nx, ny)
        out.append(("spline2 %dx%d" % (nx, ny), lambda x, y, d2=d2: d2.Prob(x, y), list(cases.queries2d(x, y))))
    return out


# ---- the kernel against numpy and scipy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", ROW_COUNTS)
def test_lookups_bit_equal_to_numpy_and_scipy(n_rows):
    from getdist_amd.colexpr import col

    todo = _all_cases()
    columns, where = [], []
    for name, fn, qs in todo:
        where.append(list(range(len(columns), len(columns) + len(qs))))
        columns += [cases.rows(q, n_rows) for q in qs]
    ctx, X = _upload(columns)
    try:
        s = Bare(ctx)
        for (name, fn, _), js in zip(todo, where):
            with np.errstate(all="ignore"):
                want = fn(*[X[:, j] for j in js])
            same_bits(fn(*[col(j) for j in js]).eval(s), want, "%s at N = %d" % (name, n_rows))
    finally:
        ctx.close()


def test_spline2_equals_scipy_ev_itself():
    """(Density2D.Prob of host vectors IS scipy's ev; said once, explicitly, on the largest grid)"""
    from scipy.interpolate import RectBivariateSpline

    from getdist_amd.colexpr import col

    d2, x, y = cases.density2d(33, 47)
    qx, qy = (cases.rows(q, N_ROWS) for q in cases.queries2d(x, y))
    ctx, X = _upload([qx, qy])
    try:
        same_bits(d2.Prob(col(0), col(1)).eval(Bare(ctx)), RectBivariateSpline(x, y, d2.P.T, s=0).ev(qx, qy), "ev")
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def abcd():
    """a weighted set whose columns a, b, c, d lie around the grids of cases.limit_tables(), with some rows outside"""
    rng = np.random.default_rng(17)
    X = rng.standard_normal((N_ROWS, 4)) * np.array([0.1, 0.5, 0.1, 0.1]) + np.array([0.0, 1.5, -0.1, -0.1])
    X[:5, :] = cases.SPECIALS[:, None]
    w = rng.integers(1, 5, N_ROWS).astype(float)
    ctx, X = _upload([X[:, j] for j in range(4)], w)
    yield Bare(ctx), X, w
    ctx.close()


def _leaves():
    from getdist_amd.colexpr import col

    return types.SimpleNamespace(**{k: col(k) for k in "abcd"})


def _host(X):
    return types.SimpleNamespace(**{k: X[:, j] for j, k in enumerate("abcd")})


def test_programs_at_the_limits_and_mixed_with_exact_ops(abcd):
    s, X, _ = abcd
    T = cases.limit_tables()
    e = cases.limits_program(_leaves(), T)
    code, consts, tables = e.compile_with_tables(s)
    assert len(code) == 128 and len(tables) == 4
    with np.errstate(all="ignore"):
        same_bits(e.eval(s), cases.limits_program(_host(X), T), "four tables, depth 16, 128 instructions")
        same_bits(cases.mixed_program(_leaves(), T).eval(s), cases.mixed_program(_host(X), T), "mixed")


def test_lookups_on_a_constant_operand(abcd):
    """a program that reads no column and needs no stack in LDS: the kernel's own dynamic LDS is then empty"""
    from getdist_amd import _lib
    from getdist_amd import colexpr as ce

    s, X, w = abcd
    p = _leaves()
    T = cases.limit_tables()
    d1, d2 = T.d1, T.d2
    zero = d1.Prob(p.a, 4)
    assert zero.kind == "const"
    xp, fp, _, _ = cases.interp_tables()["n4097"]  # 32 KiB of knots: staged, since the program itself has no LDS
    k = ce._wrap(float(d1.x[100]) + 0.004)
    for expr, want in [(d1.Prob(zero), d1.Prob(0.0)), (d1.Prob(k, 1), d1.Prob(k.args[0], 1)),
                       (np.interp(ce._wrap(0.25), xp, fp), np.interp(0.25, xp, fp)),
                       (d2.Prob(ce._wrap(float(d2.x[1])), 1.5), d2.spl.ev(d2.x[1], 1.5)),
                       (d2.Prob(zero, 1.5) > 0.0, d2.spl.ev(0.0, 1.5) > 0.0)]:
        code, consts, tables = expr.compile_with_tables(s)
        assert not (code[:, 0] == 0).any()  # no COL step
        got = expr.eval(s)
        want = np.full(N_ROWS, want, dtype=got.dtype)
        same_bits(got, want, repr(expr))
    # into the auxiliary weights and with tallies, over an odd row range
    code, consts, tables = d1.Prob(k).compile_with_tables(s)
    got, st = s.ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, lo=3, hi=1000, stats=True, tables=tables)
    v = float(d1.Prob(k.args[0]))
    same_bits(np.array(got), np.full(997, v), "range")
    assert st[0] == st[1] == v and st[2] == 997 and st[3] == 0


def test_destinations(abcd):
    from getdist_amd import _lib
    from getdist_amd.colexpr import col

    s, X, w = abcd
    ctx = s.ctx
    xp, fp, _, _ = cases.interp_tables()["n4097"]
    d2, gx, gy = cases.density2d(33, 47)
    e = np.interp(col(0) * 500.0, xp, fp) + d2.Prob(col(2) * 10.0, col(1) * 2.0)
    m = d2.Prob(col(2) * 10.0, col(1) * 2.0) > 0.2
    with np.errstate(all="ignore"):
        want = np.interp(X[:, 0] * 500.0, xp, fp) + d2.Prob(X[:, 2] * 10.0, X[:, 1] * 2.0)
        mask = d2.Prob(X[:, 2] * 10.0, X[:, 1] * 2.0) > 0.2
    assert 1000 < mask.sum() < N_ROWS - 1000
    code, consts, tables = e.compile_with_tables(s)
    cm, km, tm = m.compile_with_tables(s)

    def column(j):
        out = np.empty(ctx.N)
        ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, out.ctypes.data, ctx.column_ptr(j), out.nbytes))
        return out

    j = ctx.expr_eval(code, consts, _lib.GD_EX_TO_COLUMN, 1, tables=tables)
    assert j == ctx.n + 1
    same_bits(column(j), want, "column")
    assert e.to_column(s, 2) == ctx.n + 2
    same_bits(column(ctx.n + 2), want, "to_column")
    ld = (ctx.N + 511) // 512 * 512
    pad = np.empty(ld - ctx.N)
    ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, pad.ctypes.data, ctx.column_ptr(j) + 8 * ctx.N, pad.nbytes))
    assert not pad.any()
    # the auxiliary weights
    assert ctx.expr_eval(cm, km, _lib.GD_EX_TO_AUXW, tables=tm) is None
    ctx.select_weights(1)
    try:
        aux = np.empty(ctx.N)
        ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, aux.ctypes.data, ctx.column_ptr(-2), aux.nbytes))
        same_bits(aux, w * mask, "aux weights")
    finally:
        ctx.select_weights(0)
    # to the host: doubles and bytes, whole and over ranges with odd and even ends
    same_bits(np.array(ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, tables=tables)), want, "f64")
    u8 = np.array(ctx.expr_eval(cm, km, _lib.GD_EX_TO_HOST_U8, tables=tm))
    assert u8.dtype == np.uint8 and np.array_equal(u8, mask.astype(np.uint8))
    assert np.array_equal(m.eval(s), mask)
    for lo, hi in [(1, 2), (777, 12_346), (1001, 1514), (ctx.N - 257, ctx.N), (0, 1)]:
        same_bits(np.array(ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, lo=lo, hi=hi, tables=tables)), want[lo:hi], (lo, hi))
        assert np.array_equal(np.array(ctx.expr_eval(cm, km, _lib.GD_EX_TO_HOST_U8, lo=lo, hi=hi, tables=tm)), mask[lo:hi].astype(np.uint8))


def test_stats_and_two_runs_bit_identical(abcd):
    from getdist_amd import _lib

    s, X, _ = abcd
    T = cases.limit_tables()
    for name, fn, lo, hi in [("finite", lambda q: T.s2(q.a, q.b) - T.i1(q.c), 5, N_ROWS), ("with NaN", lambda q: T.i1(q.a) * T.s1(q.d), 0, N_ROWS),
                             ("mask", lambda q: T.s2(q.c, q.b) > 0.5, 7, N_ROWS - 3)]:
        with np.errstate(all="ignore"):
            want = np.asarray(fn(_host(X)), dtype=np.float64)[lo:hi]
        code, consts, tables = fn(_leaves()).compile_with_tables(s)
        got, st = s.ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, lo=lo, hi=hi, stats=True, tables=tables)
        got = np.array(got)
        same_bits(got, want, name)
        nn = int(np.isnan(want).sum())
        assert (name == "with NaN") == (nn > 0)
        assert st[2] == np.count_nonzero(want) and st[3] == nn, name
        if nn:
            assert np.isnan(st[0]) and np.isnan(st[1])
        else:
            assert st[0] == want.min() and st[1] == want.max(), name
        again, st2 = s.ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, lo=lo, hi=hi, stats=True, tables=tables)
        assert np.array_equal(got.view(np.uint64), np.array(again).view(np.uint64)) and np.array_equal(st.view(np.uint64), st2.view(np.uint64))


# ---- the table-free path and the argument checks --------------------------------------------------------------------------------
def _call_tab(ctx, code, consts, tabs, ntab, lo=0, hi=None):
    """gd_expr_eval_tab to host doubles with a hand-made table array; returns (return code, values)"""
    code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 2)
    consts = np.ascontiguousarray(consts, dtype=np.float64).ravel()
    hi = ctx.N if hi is None else hi
    out = ctx.pinned_array((hi - lo,), np.float64)
    rc = ctx.lib.gd_expr_eval_tab(ctx.h, code.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(code), consts.ctypes.data_as(PD),
                                  consts.size, 2, 0, lo, hi, out.ctypes.data, None,
                                  None if tabs is None else ctypes.cast(tabs, ctypes.c_void_p), ntab)
    return rc, out


def test_without_tables_the_call_is_gd_expr_eval(abcd):
    import colexpr_cases

    from getdist_amd import _lib
    from getdist_amd.colexpr import OP

    s, X, _ = abcd
    ctx = s.ctx
    for name in ("s8", "nested"):
        e = colexpr_cases.EXACT[name](_leaves())
        code, consts = e.compile(s)
        plain = np.array(ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64))
        rc, out = _call_tab(ctx, code, consts, None, 0)
        assert rc == 0
        assert np.array_equal(plain.view(np.uint64), np.array(out).view(np.uint64))
        with np.errstate(all="ignore"):
            same_bits(plain, colexpr_cases.EXACT[name](_host(X)), name)
    # the table ops stay unknown to gd_expr_eval, and to gd_expr_eval_tab without tables
    for op in sorted(_lib.GD_TAB_OPS.values()):
        bad = np.array([(OP["COL"], 0), (op, 0)], dtype=np.int32)
        with pytest.raises(_lib.GdhipError, match="unknown op") as err:
            ctx.expr_eval(bad, np.zeros(0), _lib.GD_EX_TO_HOST_F64)
        assert err.value.code == _lib.GD_ERR_BADARG
        rc, _ = _call_tab(ctx, bad, np.zeros(0), None, 0)
        assert rc == _lib.GD_ERR_BADARG and b"unknown op" in ctx.lib.gd_last_error(ctx.h)


def _raw(kind, nx, ny=0, p0=None, p1=None, p2=None, deriv=0):
    from getdist_amd import _lib

    tabs = (_lib.GdExprTable * 1)()
    t = tabs[0]
    t.kind, t.deriv, t.nx, t.ny = kind, deriv, nx, ny
    keep = []
    for name, a in (("p0", p0), ("p1", p1), ("p2", p2)):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            setattr(t, name, a.ctypes.data_as(PD))
    return tabs, keep


def test_bad_arguments_return_before_a_launch(abcd):
    from getdist_amd import _lib
    from getdist_amd.colexpr import OP, col

    s, X, _ = abcd
    ctx = s.ctx
    C = OP["COL"]
    I, S1, S2 = (_lib.GD_TAB_OPS[k] for k in ("INTERP", "SPLINE1", "SPLINE2"))
    up, z = np.arange(16.0), np.zeros(64)
    one, spl, two = [(C, 0), (I, 0)], [(C, 0), (S1, 0)], [(C, 0), (C, 1), (S2, 0)]

    def refused(code, tabs, ntab=1, **kw):
        rc, _ = _call_tab(ctx, code, np.zeros(0), None if tabs is None else tabs[0], ntab, **kw)
        assert rc == _lib.GD_ERR_BADARG
        return ctx.lib.gd_last_error(ctx.h).decode()

    down, nan, inf = up.copy(), up.copy(), up.copy()
    down[5], nan[15], inf[0] = 3.5, np.nan, -np.inf
    assert "slot" in refused([(C, 0), (I, 1)], _raw(I, 16, 0, up, z)) and "slot" in refused([(C, 0), (I, -1)], _raw(I, 16, 0, up, z))
    assert "kind" in refused(spl, _raw(I, 16, 0, up, z)) and "kind" in refused(one, _raw(S2, 8, 8, up, up, z))
    assert "table kind" in refused(one, _raw(3, 16, 0, up, z))
    assert "number of tables" in refused(one, _raw(I, 16, 0, up, z), ntab=5) and "number of tables" in refused(one, None, ntab=1)
    assert "number of tables" in refused(one, _raw(I, 16, 0, up, z), ntab=-1)
    assert "at least 1 knot" in refused(one, _raw(I, 0, 0, up, z)) and "at least 4 knots" in refused(spl, _raw(S1, 3, 0, up, z))
    assert "at least 8 knots" in refused(two, _raw(S2, 7, 8, up, up, z)) and "at least 8 knots" in refused(two, _raw(S2, 8, 7, up, up, z))
    assert "more than" in refused(one, _raw(I, 2 ** 21 + 1, 0, up, z)) and "more than" in refused(spl, _raw(S1, 2 ** 20, 0, up, z))
    assert "more than" in refused(two, _raw(S2, 2052, 2052, up, up, z))
    assert "derivative" in refused(spl, _raw(S1, 16, 0, up, z, deriv=4))
    assert "null" in refused(one, _raw(I, 16, 0, None, z)) and "null" in refused(one, _raw(I, 16, 0, up, None))
    assert "null" in refused(spl, _raw(S1, 16, 0, up, None)) and "null" in refused(two, _raw(S2, 8, 8, up, up, None))
    assert "null" in refused(two, _raw(S2, 8, 8, None, up, z)) and "null" in refused(two, _raw(S2, 8, 8, up, None, z))
    for bad in (down, nan, inf):
        assert "non-decreasing" in refused(one, _raw(I, 16, 0, bad, z)) and "non-decreasing" in refused(spl, _raw(S1, 16, 0, bad, z))
        assert "non-decreasing" in refused(two, _raw(S2, 16, 16, bad, up, z)) and "non-decreasing" in refused(two, _raw(S2, 16, 16, up, bad, z))
    assert "underflow" in refused([(I, 0)], _raw(I, 16, 0, up, z)) and "underflow" in refused([(C, 0), (S2, 0)], _raw(S2, 8, 8, up, up, z))
    assert "unknown op" in refused([(C, 0), (S2 + 1, 0)], _raw(I, 16, 0, up, z))
    assert "row range" in refused(one, _raw(I, 16, 0, up, z), lo=5, hi=5)
    # the wrapper's own errors come from compiling
    with pytest.raises(ValueError, match="non-decreasing"):
        np.interp(col(0), down, up)
    # the context still works: a plain expression and a look-up
    with np.errstate(all="ignore"):
        same_bits((col(1) * 2.0 - col(2)).eval(s), X[:, 1] * 2.0 - X[:, 2], "plain, afterwards")
    tabs, keep = _raw(I, 16, 0, up, up * up)
    tabs[0].left, tabs[0].right = 0.0, 225.0  # np.interp's defaults: fp[0] and fp[-1]
    rc, out = _call_tab(ctx, one, np.zeros(0), tabs, 1)
    assert rc == 0
    same_bits(np.array(out), np.interp(X[:, 0], up, up * up), "a hand-made table, afterwards")


# ---- end to end on an MCSamples -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets():
    """(the sample set, the 1D and 2D densities of a second, small sample set, an interpolation grid)"""
    from getdist_amd.mcsamples import MCSamples

    rng = np.random.default_rng(77)
    X = rng.standard_normal((N_ROWS, 4)) * np.array([1.0, 0.5, 1.0, 0.3]) + np.array([0.2, 0.0, 1.0, 0.5])
    w = rng.integers(1, 6, N_ROWS).astype(float)
    ll = 0.5 * np.sum((X - X.mean(axis=0)) ** 2, axis=1)
    mc = MCSamples(samples=X, weights=w, loglikes=ll, names=["x", "y", "z", "u"])
    Y = rng.standard_normal((4000, 2)) * np.array([1.2, 0.6]) + np.array([0.0, 0.1])
    other = MCSamples(samples=Y, names=["x", "y"])
    d1, d2 = other.get1DDensity("x"), other.get2DDensity("x", "y")
    d2.P  # (complete the grid)
    zg = np.linspace(-0.5, 1.5, 41)
    yield mc, d1, d2, zg, np.sqrt(zg + 1.0)
    other.ctx.close()
    mc.ctx.close()


def test_statistics_of_table_expressions(sets):
    mc, d1, d2, zg, dg = sets
    p, h = mc.getDeviceParams(), mc.getParams()
    e = d1.Prob(p.x) * np.interp(p.u, zg, dg)
    m = d2.Prob(p.x, p.y) > 0.5 * d2.P.max()
    ev, mv = e.eval(mc), m.eval(mc)
    same_bits(ev, d1.Prob(h.x) * np.interp(h.u, zg, dg), "value")
    same_bits(mv, d2.Prob(h.x, h.y) > 0.5 * d2.P.max(), "mask")
    assert 1000 < mv.sum() < N_ROWS - 1000 and np.count_nonzero(ev) > N_ROWS // 2

    def same(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))

    same(mc.mean(e), mc.mean(ev)), same(mc.var(e), mc.var(ev)), same(mc.cov([e, "x"]), mc.cov([ev, "x"]))
    same(mc.confidence(e, [0.16, 0.84]), mc.confidence(ev, [0.16, 0.84]))
    same(mc.mean(e, where=m), mc.mean(ev, where=mv)), same(mc.cov([e, "y"], where=m), mc.cov([ev, "y"], where=mv))
    same(mc.get_norm(where=m), mc.get_norm(where=mv)), same(mc.weighted_sum(e, where=m), mc.weighted_sum(ev, where=mv))
    # a composite through the device library's log, where= the contour: the same call on its host vectors
    g = np.log(d1.Prob(p.x) + 1e-3) + np.interp(p.y, zg, dg)
    gv = g.eval(mc)
    gh = np.log(d1.Prob(h.x) + 1e-3) + np.interp(h.y, zg, dg)
    assert np.all(np.abs(gv - gh) <= 4 * np.spacing(np.abs(np.log(d1.Prob(h.x) + 1e-3))) + 2 * np.spacing(np.abs(gh)))
    same(mc.mean(g, where=m), mc.mean(gv, where=mv))
    same(mc.mean("x"), mc.means[0]), same(mc.get_norm(), mc.weights.sum())


def test_mutators_take_table_expressions(sets):
    mc, d1, d2, zg, dg = sets

    def state(s):
        return s.samples, s.weights, s.loglikes, s.means, np.array(s.numrows)

    def check(do_expr, do_host):
        x, y = mc.copy(), mc.copy()
        try:
            do_expr(x, x.getDeviceParams()), do_host(y, y.getParams())
            for u, v in zip(state(x), state(y)):
                same_bits(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), "state")
            return x.numrows, x.n
        finally:
            x.ctx.close(), y.ctx.close()

    da = lambda s, p: s.addDerived(np.interp(p.u, zg, dg), "DA")  # noqa: E731
    assert check(da, da) == (N_ROWS, 5)
    level = 0.5 * d2.P.max()
    keep = lambda s, p: s.filter(d2.Prob(p.x, p.y) > level)  # noqa: E731
    assert 1000 < check(keep, keep)[0] < N_ROWS - 1000
    # the prior of another data set's marginal: the look-up is exact, so without the logarithm the two routes agree bit for bit
    prior = lambda s, p: s.reweightAddingLogLikes(1.0 - d1.Prob(p.x) / d1.P.max())  # noqa: E731
    assert check(prior, prior)[0] == N_ROWS
    # ... and with it, -log Prob, the expression equals its own host vector bit for bit, and numpy's route within the
    # device logarithm's 3 ulp plus numpy's 1 of an added log-likelihood of at most 7: 4 * 8.9e-16 = 3.6e-15 absolute in the
    # exponent of a weight, and a few roundings of 1.1e-16 in what follows: 1e-14 relative
    rw = lambda p: -np.log(d1.Prob(p.x) + 1e-3)  # noqa: E731
    x, y, z = mc.copy(), mc.copy(), mc.copy()
    try:
        x.reweightAddingLogLikes(rw(x.getDeviceParams()))
        y.reweightAddingLogLikes(rw(y.getDeviceParams()).eval(y))
        z.reweightAddingLogLikes(rw(z.getParams()))
        for u, v in zip(state(x), state(y)):
            same_bits(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), "state")
        assert np.array_equal(x.samples, z.samples) and np.allclose(x.weights, z.weights, rtol=1e-14, atol=0)
        assert np.allclose(x.loglikes, z.loglikes, rtol=0, atol=4 * np.spacing(7.0) + np.spacing(np.abs(z.loglikes).max()))
    finally:
        x.ctx.close(), y.ctx.close(), z.ctx.close()
