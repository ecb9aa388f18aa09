"""
CPU tests of the table look-ups of column expressions (np.interp, Density1D.Prob and Density2D.Prob of a ColumnExpr):
building and compiling the nodes, the checks gd_expr_eval_tab runs before a launch, and the row functions of
csrc/colexpr.hpp -- the source the kernel compiles -- built with g++ and compared BIT FOR BIT with np.interp, with this
package's Density1D.Prob of the host vector and with scipy's RectBivariateSpline.ev.  The context double is the one of
fake_ctx.py with an ``expr_eval`` that takes ``tables=`` and runs that harness over its host columns.
"""

import copy
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fake_ctx import FakeContext  # noqa: E402

from getdist_amd import _lib  # noqa: E402
from getdist_amd import colexpr as ce  # noqa: E402
from getdist_amd.colexpr import OP, ColumnExpr, col  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))
import build_colexpr  # noqa: E402
import build_coltab  # noqa: E402
import coltab_cases as cases  # noqa: E402

PI32, PD = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
TAB = _lib.GD_TAB_OPS
same_bits = cases.same_bits


@pytest.fixture(scope="module")
def harness():
    return build_coltab.load()


def _c_args(code, consts):
    code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 2)
    consts = np.ascontiguousarray(consts, dtype=np.float64).ravel()
    return code, consts, (code.ctypes.data_as(PI32), len(code), consts.ctypes.data_as(PD), consts.size)


class TabContext(FakeContext):
    """fake_ctx.FakeContext plus Context.expr_eval with ``tables=``, answered by the g++ build of csrc/colexpr.hpp"""

    lib = None

    def expr_eval(self, code, consts, dst, dst_arg=0, lo=0, hi=None, stats=False, tables=None):
        code, consts, args = _c_args(code, consts)
        hi = self.N if hi is None else hi
        cols = np.asfortranarray(self.s)
        w = None if self.w is None else np.ascontiguousarray(self.w)
        out = np.empty(self.N)
        tabs = _lib.expr_table_structs(tables or [])
        tail = (ctypes.cast(tabs, ctypes.c_void_p), len(tabs))
        rc = self.lib.coltab_run(*args, cols.shape[1], cols.ctypes.data_as(PD), None if w is None else w.ctypes.data_as(PD),
                                 self.N, out.ctypes.data_as(PD), *tail)
        if rc != 0:
            raise ValueError(self.lib.coltab_check(*args, cols.shape[1], *tail).decode())
        v = out[lo:hi]
        st = None
        if stats:
            nn = int(np.isnan(v).sum())
            st = np.array([np.nan if nn else v.min(), np.nan if nn else v.max(), np.count_nonzero(v), nn], dtype=float)
        if dst == _lib.GD_EX_TO_COLUMN:
            assert (lo, hi) == (0, self.N)
            self.s[:, self.n + dst_arg] = out
            res = self.n + dst_arg
        elif dst == _lib.GD_EX_TO_AUXW:
            assert (lo, hi) == (0, self.N) and not self._w_sel
            self._like_w = (np.ones(self.N) if self.w is None else self.w) * out
            res = None
        else:
            res = v.copy() if dst == _lib.GD_EX_TO_HOST_F64 else (v != 0).astype(np.uint8)
        return (res, st) if stats else res


class Bare:
    """What ColumnExpr needs of a sample set, over a context double that holds the given columns"""

    loglikes = None
    NAMES = ["a", "b", "c", "d"]

    def __init__(self, harness, *columns):
        TabContext.lib = harness
        self.ctx = TabContext()
        self.ctx.upload(np.column_stack(columns))
        self.n = self.ctx.n

    def _col(self, par):
        return self.NAMES.index(par) if isinstance(par, str) else int(par)


class _Stub:
    """what compiling needs of a sample set"""

    ctx = FakeContext

    def __init__(self, n=4):
        self.n = n

    def _col(self, par):
        return par if isinstance(par, int) else Bare.NAMES.index(par)


def _ops(expr):
    code, consts, tables = expr.compile_with_tables(_Stub())
    names = {v: k for k, v in TAB.items()}
    names.update(enumerate(_lib.GD_EX_OPS))
    return [(names[o], int(a)) for o, a in code], list(consts), tables


# ---- building and compiling ------------------------------------------------------------------------------------------------
def test_python_constants_match_the_header():
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gdhip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define GD_TAB_(\w+) (\d+)", text)}
    for name, code in TAB.items():
        assert defs.pop(name) == code
    assert sorted(TAB.values()) == [34, 35, 36] and min(TAB.values()) == len(_lib.GD_EX_OPS)
    assert defs.pop("MAX_TABLES") == _lib.GD_TAB_MAX_TABLES == 4 and defs.pop("MAX_DOUBLES") == _lib.GD_TAB_MAX_DOUBLES == 2 ** 22
    assert not defs
    assert not set(TAB) & set(OP) and len(_lib.GD_EX_OPS) == 34  # the GD_EX_ set is what it was


def test_interp_programs_and_stack_effects():
    a, b = col("a"), col("b")
    xp, fp = np.array([0.0, 1.0, 3.0]), np.array([1.0, -1.0, 5.0])
    e = np.interp(a, xp, fp)
    assert isinstance(e, ColumnExpr) and e.kind == "INTERP" and not e.is_bool
    ops, consts, tables = _ops(e)
    assert ops == [("COL", 0), ("INTERP", 0)] and consts == [] and len(tables) == 1
    t = tables[0]
    assert (t.kind, t.nx, t.left, t.right, t.doubles) == ("INTERP", 3, 1.0, 5.0, 6)
    assert np.array_equal(t.arrays[0], xp) and np.array_equal(t.arrays[1], fp) and not t.arrays[0].flags.writeable
    xp[0] = -9.0  # the node holds copies
    assert t.arrays[0][0] == 0.0
    xp[0] = 0.0
    e2 = ce.interp(a, xp, fp)
    ops2, _, tables2 = _ops(e2)
    assert ops2 == ops and all(np.array_equal(u, v) for u, v in zip(tables2[0].arrays, t.arrays))
    assert (tables2[0].left, tables2[0].right) == (t.left, t.right)
    t3 = _ops(np.interp(a, [0, 1], [2, 3], left=-1, right=np.inf))[2][0]  # lists, integers, left and right
    assert (t3.left, t3.right, t3.arrays[1].dtype) == (-1.0, np.inf, np.float64)
    # the operand is any float expression; the result an ordinary float node
    ops, consts, tables = _ops(np.log(np.interp(a * 2.0 + b, xp, fp)) > 0.5)
    assert ops == [("COL", 0), ("CONST", 0), ("MUL", 0), ("COL", 1), ("ADD", 0), ("INTERP", 0), ("LOG", 0), ("CONST", 1), ("GT", 0)]
    assert "interp table 3" in repr(e) and "1." not in repr(e).replace("col", "")  # kind and shape, not the contents


def test_density_nodes_and_stack_effects():
    a, b = col("a"), col("b")
    d1, x = cases.density1d(5)
    e = d1.Prob(a)
    ops, _, tables = _ops(e)
    assert ops == [("COL", 0), ("SPLINE1", 0)] and (tables[0].kind, tables[0].nx, tables[0].deriv) == ("SPLINE1", 5, 0)
    assert tables[0].arrays[1].shape == (4, 4) and tables[0].doubles == 5 + 16
    assert _ops(d1(a))[2][0] is tables[0]  # __call__ is Prob; one Table per density and derivative
    assert _ops(d1.Prob(a, 2))[2][0].deriv == 2 and _ops(d1.Prob(a, derivative=3))[2][0].deriv == 3
    for d in (4, 5):
        z = d1.Prob(a, d)
        assert z.kind == "const" and z.args == (0.0,)
    # the coefficients are the ones the host path evaluates
    y, c1, c2, c3 = d1.spl.coefficients()
    assert np.array_equal(tables[0].arrays[1], np.stack([y, c1, c2, c3], axis=1)) and np.array_equal(y, d1.P[:-1])
    d2, gx, gy = cases.density2d(5, 9)
    e = d2.Prob(a, b)
    ops, _, tables = _ops(e)
    assert ops == [("COL", 0), ("COL", 1), ("SPLINE2", 0)]  # pops y, then x
    t = tables[0]
    tx, ty, c = d2.spl.tck
    assert (t.kind, t.nx, t.ny) == ("SPLINE2", 9, 13) and all(np.array_equal(u, v) for u, v in zip(t.arrays, (tx, ty, c)))
    assert "spline2 table 5x9" in repr(e)
    # a scalar for one argument; __call__; a comparison on top
    ops, consts, _ = _ops(d2(a, 1.5) > 0.25)
    assert ops == [("COL", 0), ("CONST", 0), ("SPLINE2", 0), ("CONST", 1), ("GT", 0)] and consts == [1.5, 0.25]
    assert _ops(d2.Prob(2, b))[0] == [("CONST", 0), ("COL", 1), ("SPLINE2", 0)]
    # depth: SPLINE2 takes two entries and leaves one
    code, consts, tables = (d2.Prob(a, b) + d2.Prob(b, a)).compile_with_tables(_Stub())
    assert len(tables) == 1 and [int(o) for o in code[:, 0]] == [0, 0, TAB["SPLINE2"], 0, 0, TAB["SPLINE2"], OP["ADD"]]
    # the host call is what it was
    assert isinstance(d2.Prob(0.1, 1.5), np.ndarray) and isinstance(d1.Prob(0.1), float) and d1.Prob([0.1]).shape == (1,)


def test_shared_tables_and_the_limits(harness):
    a = col("a")
    xp, fp = np.arange(4.0), np.arange(4.0) ** 2
    e = np.interp(a, xp, fp)
    twice = e * np.interp(a + 1.0, xp, fp)  # equal contents, two payloads: two slots
    assert [op for op in _ops(twice)[0] if op[0] == "INTERP"] == [("INTERP", 0), ("INTERP", 1)]
    shared = ce.lookup("INTERP", e.args[-1], a + 1.0) * e + e  # the same payload: one slot
    ops, _, tables = _ops(shared)
    assert [op for op in ops if op[0] == "INTERP"] == [("INTERP", 0)] * 3 and len(tables) == 1
    four = sum((np.interp(a, xp + k, fp) for k in range(1, 4)), np.interp(a, xp, fp))
    assert len(_ops(four)[2]) == 4 == _lib.GD_TAB_MAX_TABLES
    code, consts, tables = four.compile_with_tables(_Stub())
    _, _, args = _c_args(code, consts)
    tabs = _lib.expr_table_structs(tables)
    assert harness.coltab_check(*args, 8, ctypes.cast(tabs, ctypes.c_void_p), 4) is None
    assert harness.coltab_depth(*args, 8, ctypes.cast(tabs, ctypes.c_void_p), 4) == 2
    with pytest.raises(ValueError, match="distinct tables .at most 4"):
        (four + np.interp(a, xp + 9, fp)).compile_with_tables(_Stub())
    # 2^22 doubles fit, one more pair does not (an interpolation table holds xp and fp)
    big = np.arange(2.0 ** 21)
    assert _ops(np.interp(a, big, big))[2][0].doubles == 2 ** 22
    big = np.arange(2.0 ** 21 + 1)
    with pytest.raises(ValueError, match="doubles .at most 4194304"):
        np.interp(a, big, big).compile_with_tables(_Stub())
    # the limits of the table-free program hold as before
    with pytest.raises(ValueError, match="instructions"):
        x = e
        for _ in range(127):
            x = -x
        x.compile_with_tables(_Stub())


def test_what_building_refuses():
    a = col("a")
    xp, fp = np.arange(4.0), np.arange(4.0)
    with pytest.raises(TypeError, match="period"):
        np.interp(a, xp, fp, period=2.0)
    with pytest.raises(TypeError, match="host arrays"):
        np.interp(a, a, fp)
    with pytest.raises(TypeError, match="host arrays"):
        np.interp(a, xp, a)
    with pytest.raises(TypeError, match="column expression"):
        ce.interp(np.zeros(3), xp, fp)
    with pytest.raises(ValueError, match="non-decreasing"):
        np.interp(a, [0.0, 2.0, 1.0], [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="non-decreasing"):
        np.interp(a, [0.0, np.nan, 1.0], [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="finite"):
        np.interp(a, [0.0, 1.0, np.inf], [0.0, 0.0, 0.0])
    for bad in (([], []), ([1.0, 2.0], [1.0]), (np.zeros((2, 2)), np.zeros((2, 2)))):
        with pytest.raises(ValueError, match="1-D"):
            np.interp(a, *bad)
    d1, _ = cases.density1d(5)
    d2, _, _ = cases.density2d(4, 4)
    with pytest.raises(TypeError, match="grid=True"):
        d2.Prob(a, col("b"), grid=True)
    with pytest.raises(TypeError, match="grid=True"):
        d2(a, 0.5, grid=True)
    with pytest.raises(TypeError, match="dx"):
        d2(a, 0.5, dx=1)
    with pytest.raises(TypeError, match="host array"):
        d2.Prob(a, np.zeros(3))
    with pytest.raises(TypeError):
        d1.Prob(a > 0, a)  # (a derivative order is a number)
    t = np.interp(a, xp, fp).args[-1]
    with pytest.raises(AttributeError):
        t.left = 1.0
    with pytest.raises(ValueError):
        t.arrays[0][0] = 1.0


def test_lookups_on_a_constant_operand(harness):
    """A program whose only pushes are constants reads no column and needs no stack in memory: the fourth derivative of
    a density is such a constant, and a look-up of it is a valid program."""
    a = col("a")
    d1, x = cases.density1d(5)
    d2, gx, gy = cases.density2d(4, 4)
    zero = d1.Prob(a, 4)
    assert zero.kind == "const"
    e = d1.Prob(zero)
    code, consts, tables = e.compile_with_tables(_Stub())
    assert [tuple(c) for c in code] == [(OP["CONST"], 0), (TAB["SPLINE1"], 0)] and list(consts) == [0.0]
    _, _, args = _c_args(code, consts)
    tabs = _lib.expr_table_structs(tables)
    assert harness.coltab_check(*args, 8, ctypes.cast(tabs, ctypes.c_void_p), 1) is None
    assert harness.coltab_depth(*args, 8, ctypes.cast(tabs, ctypes.c_void_p), 1) == 1
    s = Bare(harness, np.linspace(-1, 1, 9))
    xp, fp = np.array([0.0, 1.0, 3.0]), np.array([1.0, -1.0, 5.0])
    k = ce._wrap(float(x[2]) + 0.004)
    for expr, want in [(e, d1.Prob(0.0)), (d1.Prob(k, 1), d1.Prob(k.args[0], 1)), (np.interp(ce._wrap(0.25), xp, fp), np.interp(0.25, xp, fp)),
                       (d2.Prob(ce._wrap(float(gx[1])), 1.5), d2.spl.ev(gx[1], 1.5)), (d2.Prob(zero, a * 0.0 + 1.5), d2.spl.ev(0.0, 1.5))]:
        same_bits(expr.eval(s), np.full(9, float(want)), repr(expr))


def test_compile_points_to_compile_with_tables():
    a = col("a")
    e = np.interp(a, [0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="compile_with_tables"):
        e.compile(_Stub())
    with pytest.raises(ValueError, match="compile_with_tables"):
        (np.sqrt(e) + 1.0).compile(_Stub())
    plain = a * 2.0
    pair = plain.compile(_Stub())
    assert len(pair) == 2
    code, consts, tables = plain.compile_with_tables(_Stub())
    assert np.array_equal(code, pair[0]) and np.array_equal(consts, pair[1]) and tables == []


def test_run_passes_tables_only_when_there_are(harness):
    s = Bare(harness, np.linspace(-1, 2, 7))
    seen = []
    real = s.ctx.expr_eval
    s.ctx.expr_eval = lambda *a, **k: (seen.append(sorted(k)), real(*a, **k))[1]
    (col(0) * 2.0).eval(s)
    np.interp(col(0), [0.0, 1.0], [0.0, 1.0]).eval(s)
    assert seen == [[], ["tables"]]
    share = object()
    s._column_share = share
    from getdist_amd.chains import MCSamplesError

    with pytest.raises(MCSamplesError, match="share of the columns"):
        np.interp(col(0), [0.0, 1.0], [0.0, 1.0]).eval(s)


# ---- the checks of the entry point --------------------------------------------------------------------------------------------
def _raw(kind, nx, ny=0, p0=None, p1=None, p2=None, deriv=0):
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


def test_native_check_refuses_what_the_entry_point_must(harness):
    C = OP["COL"]
    I, S1, S2 = TAB["INTERP"], TAB["SPLINE1"], TAB["SPLINE2"]
    up, z = np.arange(16.0), np.zeros(64)

    def check(code, tabs, ntab=None):
        _, _, args = _c_args(np.array(code, dtype=np.int32), np.zeros(0))
        arr = tabs[0] if tabs else None
        n = (len(arr) if arr is not None else 0) if ntab is None else ntab
        return harness.coltab_check(*args, 8, ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, n)

    one, two = [(C, 0), (I, 0)], [(C, 0), (C, 1), (S2, 0)]
    assert check(one, _raw(I, 16, 0, up, z)) is None and check(one, _raw(I, 1, 0, up, z)) is None
    assert check([(C, 0), (S1, 0)], _raw(S1, 4, 0, up, z)) is None and check([(C, 0), (S1, 0)], _raw(S1, 16, 0, up, z, deriv=3)) is None
    assert check(two, _raw(S2, 8, 8, up, up, z)) is None and check(two, _raw(S2, 16, 12, up, up, z * np.ones((2, 1)))) is None
    # the table ops without tables are unknown ops: the table-free check, and the old harness
    for op in (I, S1, S2):
        assert b"unknown op" in check([(C, 0), (op, 0)], None)
    old = build_colexpr.load()
    for op in (I, S1, S2, S2 + 1):
        _, _, args = _c_args(np.array([(C, 0), (op, 0)], dtype=np.int32), np.zeros(0))
        assert b"unknown op" in old.colexpr_check(*args, 8)
    assert b"unknown op" in check([(C, 0), (S2 + 1, 0)], _raw(I, 16, 0, up, z))
    # slot, kind, stack
    assert b"slot" in check([(C, 0), (I, 1)], _raw(I, 16, 0, up, z)) and b"slot" in check([(C, 0), (I, -1)], _raw(I, 16, 0, up, z))
    assert b"kind" in check([(C, 0), (S1, 0)], _raw(I, 16, 0, up, z)) and b"kind" in check(one, _raw(S1, 16, 0, up, z))
    assert b"kind" in check(one, _raw(S2, 8, 8, up, up, z)) and b"table kind" in check(one, _raw(7, 16, 0, up, z))
    assert b"underflow" in check([(I, 0)], _raw(I, 16, 0, up, z)) and b"underflow" in check([(C, 0), (S2, 0)], _raw(S2, 8, 8, up, up, z))
    assert b"exactly one" in check([(C, 0), (C, 1), (I, 0)], _raw(I, 16, 0, up, z))
    # number of tables
    assert b"number of tables" in check(one, _raw(I, 16, 0, up, z), ntab=5) and b"number of tables" in check(one, _raw(I, 16, 0, up, z), ntab=-1)
    assert b"number of tables" in check(one, None, ntab=1)
    # sizes below the minimum and above the limit
    assert b"at least 1 knot" in check(one, _raw(I, 0, 0, up, z))
    assert b"at least 4 knots" in check([(C, 0), (S1, 0)], _raw(S1, 3, 0, up, z))
    assert b"at least 8 knots" in check(two, _raw(S2, 7, 8, up, up, z)) and b"at least 8 knots" in check(two, _raw(S2, 8, 7, up, up, z))
    assert b"more than" in check(one, _raw(I, 2 ** 21 + 1, 0, up, z))
    assert b"more than" in check([(C, 0), (S1, 0)], _raw(S1, (2 ** 22 + 4) // 5 + 1, 0, up, z))
    assert b"more than" in check(two, _raw(S2, 2052, 2052, up, up, z)) and b"more than" in check(two, _raw(S2, 2 ** 31 - 1, 2 ** 31 - 1, up, up, z))
    assert b"derivative" in check([(C, 0), (S1, 0)], _raw(S1, 16, 0, up, z, deriv=4))
    assert b"derivative" in check([(C, 0), (S1, 0)], _raw(S1, 16, 0, up, z, deriv=-1))
    # null pointers
    assert b"null" in check(one, _raw(I, 16, 0, None, z)) and b"null" in check(one, _raw(I, 16, 0, up, None))
    assert b"null" in check([(C, 0), (S1, 0)], _raw(S1, 16, 0, up, None))
    for k in range(3):
        ptrs = [up, up, z]
        ptrs[k] = None
        assert b"null" in check(two, _raw(S2, 8, 8, *ptrs))
    # knots: non-decreasing and finite (equal ones are fine)
    down, nan, inf = up.copy(), up.copy(), up.copy()
    down[5], nan[15], inf[0] = 3.5, np.nan, -np.inf
    eq = np.repeat(np.arange(8.0), 2)
    assert check(one, _raw(I, 16, 0, eq, z)) is None and check(two, _raw(S2, 16, 16, eq, eq, z)) is None
    for bad in (down, nan, inf):
        assert b"non-decreasing" in check(one, _raw(I, 16, 0, bad, z))
        assert b"non-decreasing" in check([(C, 0), (S1, 0)], _raw(S1, 16, 0, bad, z))
        assert b"non-decreasing" in check(two, _raw(S2, 16, 16, bad, up, z)) and b"non-decreasing" in check(two, _raw(S2, 16, 16, up, bad, z))
    assert check(one, _raw(I, 5, 0, down, z)) is None  # only the nx knots count


# ---- the row functions against numpy, the host spline and scipy, bit for bit -------------------------------------------------------
def test_interval_search_equals_searchsorted(harness):
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 257, 4097):
        t = np.sort(np.round(rng.uniform(0, n / 3 + 1, n) * 4) / 4)  # many ties
        q = cases.queries(t, 301)
        for lo, hi in ((0, n), (n // 3, n - n // 4), (n // 2, n // 2)):
            want = np.searchsorted(t[lo:hi], q, side="right") + lo
            want[np.isnan(q)] = hi
            got = np.array([harness.coltab_upper(t.ctypes.data_as(PD), lo, hi, v) for v in q])
            assert np.array_equal(got, want), (n, lo, hi)


@pytest.mark.parametrize("name", sorted(cases.interp_tables()))
def test_interp_bit_equal_to_numpy(harness, name):
    xp, fp, left, right = cases.interp_tables()[name]
    q = cases.queries(xp)
    with np.errstate(all="ignore"):
        want = np.interp(q, xp, fp, left=left, right=right)
        got = np.interp(col(0), xp, fp, left=left, right=right).eval(Bare(harness, q))
    if len(xp) > 1:
        assert np.array_equal(np.isnan(want), np.isnan(q)) or not np.all(np.isfinite(fp)) or right is not None
    same_bits(got, want, name)


def test_interp_rescue_branch_with_infinite_knots(harness):
    """Knots of +-inf make slope * (x - xp[j]) the NaN 0 * inf for a finite x: numpy then retries from the right-hand knot and,
    if that is NaN too, takes fp[j] where both ends are equal.  The entry point refuses such knots, so this runs the row
    function on its own."""
    for xp, fp in [([-np.inf, 0.0, 1.0], [2.0, 2.0, 3.0]), ([-np.inf, 0.0, np.inf], [2.0, 2.0, 2.0]),
                   ([-np.inf, np.inf], [1.5, 1.5]), ([-np.inf, np.inf], [1.0, 2.0]), ([0.0, 1.0, np.inf], [1.0, 2.0, 2.0])]:
        xp, fp = np.array(xp), np.array(fp)
        q = np.array([-np.inf, -5.0, -0.0, 0.0, 0.5, 1.0, 7.0, np.inf, np.nan])
        with np.errstate(all="ignore"):
            want = np.interp(q, xp, fp)
        tabs, keep = _raw(TAB["INTERP"], len(xp), 0, xp, fp)
        tabs[0].left, tabs[0].right = fp[0], fp[-1]
        got = np.empty_like(q)
        harness.coltab_rows(ctypes.cast(tabs, ctypes.c_void_p), q.ctypes.data_as(PD), q.ctypes.data_as(PD), len(q), got.ctypes.data_as(PD))
        same_bits(got, want, (list(xp), list(fp)))


@pytest.mark.parametrize("n", [k for k in cases.KNOT_COUNTS if k >= 4])
def test_density1d_prob_bit_equal_to_the_host_vector(harness, n):
    d1, x = cases.density1d(n)
    q = cases.queries(x)
    s = Bare(harness, q)
    for d in (0, 1, 2, 3, 4):
        with np.errstate(all="ignore"):
            want = d1.Prob(q, d)
            got = d1.Prob(col(0), d).eval(s)
        same_bits(got, want, (n, d))
        if d < 3:
            assert np.isnan(got[np.isnan(q)]).all() and not got[(q < x[0]) | (q > x[-1])].any()
    same_bits(d1(col(0)).eval(s), d1(q), "call")


@pytest.mark.parametrize("nx,ny", cases.GRIDS)
def test_density2d_prob_bit_equal_to_scipy_ev(harness, nx, ny):
    from scipy.interpolate import RectBivariateSpline

    d2, x, y = cases.density2d(nx, ny)
    qx, qy = cases.queries2d(x, y)
    want = RectBivariateSpline(x, y, d2.P.T, s=0).ev(qx, qy)
    s = Bare(harness, qx, qy)
    same_bits(d2.Prob(col(0), col(1)).eval(s), want, (nx, ny))
    same_bits(d2.Prob(col(0), col(1)).eval(s), d2.Prob(qx, qy), "the package's own host call")
    assert np.array_equal(np.isnan(want), np.isnan(qx) | np.isnan(qy))
    # a scalar on one side
    same_bits(d2.Prob(col(0), float(y[1])).eval(s), d2.spl.ev(qx, np.full_like(qx, y[1])), "scalar y")
    same_bits(d2(float(x[2]), col(1)).eval(s), d2.spl.ev(np.full_like(qy, x[2]), qy), "scalar x")


def test_programs_at_the_limits_and_mixed_with_exact_ops(harness):
    """the programs the GPU tier runs: four tables, a stack 16 deep, 128 instructions; look-ups among the exact ops"""
    import types

    rng = np.random.default_rng(17)
    X = rng.standard_normal((2003, 4)) * np.array([0.1, 0.5, 0.1, 0.1]) + np.array([0.0, 1.5, -0.1, -0.1])
    X[:5, :] = cases.SPECIALS[:, None]
    s = Bare(harness, *X.T)
    T = cases.limit_tables()
    p = types.SimpleNamespace(**{k: col(k) for k in "abcd"})
    h = types.SimpleNamespace(**{k: X[:, j] for j, k in enumerate("abcd")})
    e = cases.limits_program(p, T)
    code, consts, tables = e.compile_with_tables(s)
    _, _, args = _c_args(code, consts)
    tabs = _lib.expr_table_structs(tables)
    assert len(code) == 128 and len(tables) == 4 and harness.coltab_depth(*args, 8, ctypes.cast(tabs, ctypes.c_void_p), 4) == 16
    with np.errstate(all="ignore"):
        same_bits(e.eval(s), cases.limits_program(h, T), "limits")
        same_bits(cases.mixed_program(p, T).eval(s), cases.mixed_program(h, T), "mixed")


# ---- composition and the places that take an expression -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def setup(harness):
    """(sample set on the context double, d1 and d2 of a second small sample-like grid, interp arrays)"""
    from getdist_amd.mcsamples import MCSamples

    TabContext.lib = harness
    rng = np.random.default_rng(41)
    X = rng.standard_normal((997, 4)) * np.array([0.05, 0.3, 1.0, 1.0]) + np.array([-0.05, 1.8, 0.0, 0.0])
    mc = MCSamples(samples=X, weights=rng.integers(1, 5, len(X)).astype(float), loglikes=rng.standard_normal(len(X)) ** 2,
                   names=Bare.NAMES, _context_factory=TabContext)
    d1, _ = cases.density1d(33)  # grid -0.37 .. 0.05: most of column a inside, some outside
    d2, _, _ = cases.density2d(5, 9)  # x -0.21 .. 0.07, y 1.3 .. 2.18
    zg = np.linspace(1.0, 2.5, 21)
    return mc, d1, d2, zg, np.sqrt(zg) - 1.0


def _exprs(p, d1, d2, zg, dg):
    value = np.log(d1.Prob(p.a) + 1.0) + np.interp(p.b, zg, dg)
    mask = d2.Prob(p.a, p.b) > 0.3
    return value, mask


def test_composition_equals_the_host_vectors(setup):
    """The look-ups are exact, np.log is the C library's here (the device library's on the GPU): the composite is compared
    with numpy within 2 ulp, its exact parts bit for bit, and every statistic of the expression with the same call given the
    host vectors it evaluates to -- with ==, as tests/test_colexpr_cpu.py compares them."""
    mc, d1, d2, zg, dg = setup
    p, h = mc.getDeviceParams(), mc.getParams()
    e, m = _exprs(p, d1, d2, zg, dg)
    eh, mh = _exprs(h, d1, d2, zg, dg)
    assert isinstance(e, ColumnExpr) and not e.is_bool and m.is_bool and isinstance(eh, np.ndarray)
    ev, mv = e.eval(mc), m.eval(mc)
    same_bits(mv, mh, "mask")
    same_bits((d1.Prob(p.a) + 1.0 - np.interp(p.b, zg, dg)).eval(mc), d1.Prob(h.a) + 1.0 - np.interp(h.b, zg, dg), "exact parts")
    assert np.all(np.abs(ev - eh) <= 2 * np.spacing(np.abs(eh)))
    assert mv.dtype == bool and 100 < mv.sum() < len(mv) - 100 and 500 < np.count_nonzero(d1.Prob(h.a)) < len(mv)
    assert len(e.compile_with_tables(mc)[2]) == 2 and len(np.where(m, e, -e).compile_with_tables(mc)[2]) == 3
    assert mc.mean(e, where=m) == mc.mean(ev, where=mv) and mc.var(e, where=m) == mc.var(ev, where=mv)
    assert np.array_equal(mc.cov([e, "d"], where=m), mc.cov([ev, "d"], where=mv))
    assert mc.get_norm(where=m) == mc.weights[mh].sum()
    assert np.array_equal(mc.confidence(e, [0.16, 0.84]), mc.confidence(ev, [0.16, 0.84]))
    assert mc.weighted_sum(e) == mc.weighted_sum(ev)


def test_mutators_take_table_expressions(setup):
    mc0, d1, d2, zg, dg = setup

    def state(mc):
        return mc.samples, mc.weights, mc.loglikes, np.array(mc.numrows, dtype=float)

    def check(do):
        x, y = mc0.copy(), mc0.copy()
        do(x, _exprs(x.getDeviceParams(), d1, d2, zg, dg))
        do(y, [v.eval(y) for v in _exprs(y.getDeviceParams(), d1, d2, zg, dg)])  # the host route: vectors
        for u, v in zip(state(x), state(y)):
            same_bits(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), "state")
        return x.numrows, x.n

    assert check(lambda s, ex: s.addDerived(ex[0], "DA")) == (997, 5)
    assert check(lambda s, ex: s.reweightAddingLogLikes(-ex[0]))[0] == 997
    assert 100 < check(lambda s, ex: s.filter(ex[1]))[0] < 897

    # without the logarithm the look-ups are exact, and the host route is numpy's and scipy's own: vectors built from
    # getParams() columns, independent of the harness
    def exact(p):
        return 1.0 - d1.Prob(p.a) / d1.P.max() + np.interp(p.b, zg, dg), d2.Prob(p.a, p.b) > 0.3

    def check_numpy(do):
        x, y = mc0.copy(), mc0.copy()
        do(x, exact(x.getDeviceParams()))
        do(y, exact(y.getParams()))
        assert isinstance(exact(y.getParams())[0], np.ndarray)
        for u, v in zip(state(x), state(y)):
            same_bits(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), "state")
        return x.numrows, x.n

    assert check_numpy(lambda s, ex: s.addDerived(ex[0], "DA")) == (997, 5)
    assert check_numpy(lambda s, ex: s.reweightAddingLogLikes(ex[0]))[0] == 997
    assert 100 < check_numpy(lambda s, ex: s.filter(ex[1]))[0] < 897


def test_table_expressions_copy_and_pickle(setup):
    mc, d1, d2, zg, dg = setup
    p = mc.getDeviceParams()
    e, m = _exprs(p, d1, d2, zg, dg)
    both = np.where(m, e, d1.Prob(p.a) * 2.0)  # d1's table twice: one slot
    assert len(both.compile_with_tables(mc)[2]) == 3
    assert copy.copy(both) is both and copy.deepcopy(both) is both
    for x in (e, m, both):
        y = pickle.loads(pickle.dumps(x))
        assert isinstance(y, ColumnExpr) and y is not x and repr(y) == repr(x) and y.is_bool == x.is_bool
        assert y.args[-1] is not x.args[-1] or not isinstance(x.args[-1], ce.Table)  # the tables travel with the node
        same_bits(y.eval(mc), x.eval(mc), "pickled")
        assert len(y.compile_with_tables(mc)[2]) == len(x.compile_with_tables(mc)[2])  # sharing survives
    t = e.args[0].args[0].args[0].args[-1]
    assert isinstance(t, ce.Table) and copy.deepcopy(t).arrays[0].flags.writeable is False


def test_one_table_expression_on_two_sample_sets(setup, harness):
    from getdist_amd.mcsamples import MCSamples

    mc, d1, d2, zg, dg = setup
    rng = np.random.default_rng(43)
    s = rng.standard_normal((50, 3)) * 0.1
    other = MCSamples(samples=s, names=["b", "zz", "a"], _context_factory=TabContext)
    e = d1.Prob(col("a")) - np.interp(col("b"), zg, dg)
    same_bits(e.eval(mc), d1.Prob(mc.samples[:, 0]) - np.interp(mc.samples[:, 1], zg, dg), "first")
    same_bits(e.eval(other), d1.Prob(s[:, 2]) - np.interp(s[:, 0], zg, dg), "second")
