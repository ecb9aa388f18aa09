"""GPU tier of column expressions: gd_expr_eval through Context.expr_eval (every op alone and the composites of the CPU test
against numpy on the host copy, the four destinations, the tallies, the argument checks), the transcendental ops against
an extended-precision truth, and expressions end to end on an MCSamples.

Exact class (+ - * / sqrt square reciprocal negative absolute minimum maximum, comparisons, logic, where): BIT-EQUAL to
numpy (uint64 views; NaNs compared as NaN-ness).  minimum / maximum of the tallies are compared with ==: which of -0.0
and +0.0 a reduction returns depends on its order, in numpy as well.

Transcendental class: the truth is the np.longdouble evaluation where that type has a 63-bit mantissa (x86), mpmath at
113 bits otherwise; the error is counted in np.spacing of the rounded truth, and the cap per function is OpenCL 3.0's bound for double precision
(section 7.4, "Relative error as ULPs"), which the ROCm device library is written to meet: exp log log10 log2 3, sin cos
4, tan atan tanh 5, atan2 6, pow 16.  No document installed with the ROCm tree states a bound for double, so these stand.
The cap catches a wrong function, swapped arguments or single-precision evaluation; it does not rank accuracy.  numpy's own
error on the same inputs is printed beside the device's (run with -s; profiles/colexpr_gpu_tests.txt keeps one such run).
"""

import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colexpr_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
N_ROWS = 20_011  # not a multiple of 64, 256 or 512
N_COLS = 20


class Bare:
    """What ColumnExpr needs of a sample set, over a bare Context: columns a, b, c, d are 0..3, others by index."""

    loglikes = None

    def __init__(self, ctx):
        self.ctx, self.n = ctx, ctx.n

    def _col(self, par):
        return cases.NAMES.index(par) if isinstance(par, str) else int(par)


def _leaves():
    from getdist_amd.colexpr import col

    return types.SimpleNamespace(**{k: col(k) for k in cases.NAMES})


def _host(X):
    return types.SimpleNamespace(**{k: X[:, j] for j, k in enumerate(cases.NAMES)})


def _make(n_rows, weighted, seed):
    from getdist_amd._lib import Context

    X4, w, _ = cases.inputs(max(n_rows - 256, 0), seed)
    X4, w = X4[len(X4) - n_rows:], w[len(w) - n_rows:]  # (the specials are the last rows: the small sets are made of them)
    rng = np.random.default_rng(seed + 1)
    X = np.asfortranarray(np.hstack([X4, rng.standard_normal((n_rows, N_COLS - 4))]))
    ctx = Context(0)
    ctx.upload(X, w if weighted else None)
    return ctx, X, (w if weighted else None)


@pytest.fixture(scope="module")
def weighted():
    ctx, X, w = _make(N_ROWS, True, 7)
    yield Bare(ctx), X, w
    ctx.close()


@pytest.fixture(scope="module")
def unit():
    ctx, X, _ = _make(N_ROWS, False, 8)
    yield Bare(ctx), X, None
    ctx.close()


# ---- gd_expr_eval: the exact class ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.EXACT) + sorted(cases.COMPOSITES))
def test_exact_ops_bit_equal_to_numpy(weighted, name):
    s, X, _ = weighted
    fn = cases.EXACT.get(name) or cases.COMPOSITES[name]
    with np.errstate(all="ignore"):
        want = fn(_host(X))
    cases.same_bits(fn(_leaves()).eval(s), want, name)


@pytest.mark.parametrize("n_rows", [1, 63, 513])
def test_one_op_programs_at_small_row_counts(n_rows):
    ctx, X, w = _make(n_rows, True, 9)
    try:
        s = Bare(ctx)
        for name in cases.ONE_OP:
            with np.errstate(all="ignore"):
                want = cases.EXACT[name](_host(X))
            cases.same_bits(cases.EXACT[name](_leaves()).eval(s), want, "%s at N = %d" % (name, n_rows))
    finally:
        ctx.close()


def test_destinations(weighted, unit):
    from getdist_amd import _lib
    from getdist_amd.colexpr import col, weights

    for s, X, w in (weighted, unit):
        ctx, p = s.ctx, _leaves()
        e = p.a * np.sqrt(abs(p.b) / 0.3) - p.c
        with np.errstate(all="ignore"):
            want = X[:, 0] * np.sqrt(abs(X[:, 1]) / 0.3) - X[:, 2]
        code, consts = e.compile(s)

        def column(j):
            out = np.empty(ctx.N)
            ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, out.ctypes.data, ctx.column_ptr(j), out.nbytes))
            return out

        # a spare column, read back; then in place: the slot the program reads is the slot it writes
        j = ctx.expr_eval(code, consts, _lib.GD_EX_TO_COLUMN, 1)
        assert j == ctx.n + 1
        cases.same_bits(column(j), want, "column")
        code2, consts2 = (col(j) * 2.0 - col(0)).compile(s)
        assert ctx.expr_eval(code2, consts2, _lib.GD_EX_TO_COLUMN, 1) == j
        with np.errstate(all="ignore"):
            cases.same_bits(column(j), want * 2.0 - X[:, 0], "in place")
        # ... and the padding behind row N stays zero
        ld = (ctx.N + 511) // 512 * 512
        pad = np.empty(ld - ctx.N)
        ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, pad.ctypes.data, ctx.column_ptr(j) + 8 * ctx.N, pad.nbytes))
        assert not pad.any()

        # the auxiliary weights: host w * mask bit for bit (read through the weights leaf while they are selected? no:
        # that leaf always means the SAMPLE weights -- so through the norm and a cov under them, and a raw copy)
        m = (p.d > 0.0) & ~(p.a < -1)
        mask = (X[:, 3] > 0.0) & ~(X[:, 0] < -1)
        cm, km = m.compile(s)
        assert ctx.expr_eval(cm, km, _lib.GD_EX_TO_AUXW) is None
        ctx.select_weights(1)
        try:
            aux = np.empty(ctx.N)
            ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, aux.ctypes.data, ctx.column_ptr(-2), aux.nbytes))
            cases.same_bits(aux, (np.ones(ctx.N) if w is None else w) * mask, "aux weights")
            cases.same_bits(weights.eval(s), np.ones(ctx.N) if w is None else w, "the weights leaf under auxiliary weights")
            with pytest.raises(_lib.GdhipError):  # refused while they are selected
                ctx.expr_eval(cm, km, _lib.GD_EX_TO_AUXW)
        finally:
            ctx.select_weights(0)

        # to the host, whole and over sub-ranges with odd and even ends
        cases.same_bits(np.array(ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64)), want, "f64")
        u8 = np.array(ctx.expr_eval(cm, km, _lib.GD_EX_TO_HOST_U8))
        assert u8.dtype == np.uint8 and np.array_equal(u8, mask.astype(np.uint8))
        for lo, hi in [(1, 2), (777, 12_346), (1000, 1513), (ctx.N - 257, ctx.N), (ctx.N - 1, ctx.N), (0, 1)]:
            cases.same_bits(np.array(ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, lo=lo, hi=hi)), want[lo:hi], (lo, hi))
            assert np.array_equal(np.array(ctx.expr_eval(cm, km, _lib.GD_EX_TO_HOST_U8, lo=lo, hi=hi)), mask[lo:hi].astype(np.uint8))
        # a float program fetched as bytes: value != 0, NaN included
        with np.errstate(all="ignore"):
            assert np.array_equal(np.array(ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_U8)), (want != 0).astype(np.uint8))


def test_stats_equal_numpy(weighted):
    from getdist_amd import _lib

    s, X, _ = weighted
    p, h = _leaves(), _host(X)
    for name, fn, lo, hi in [("finite", lambda q: np.minimum(np.maximum(q.c, -1e3), 1e3) * (q.d > 0), 0, N_ROWS - 256),
                             ("with NaN", lambda q: q.a - q.b, 0, N_ROWS),
                             ("mask", lambda q: (q.a > 0) & (q.b < 1), 5, N_ROWS - 3),
                             ("one row", lambda q: q.a + 1.0, 11, 12)]:
        with np.errstate(all="ignore"):
            want = np.asarray(fn(h), dtype=np.float64)[lo:hi]
        code, consts = fn(p).compile(s)
        got, st = s.ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, lo=lo, hi=hi, stats=True)
        cases.same_bits(np.array(got), want, name)
        nn = int(np.isnan(want).sum())
        assert (name == "with NaN") == (nn > 0)
        assert st[2] == np.count_nonzero(want) and st[3] == nn, name
        if nn:
            assert np.isnan(st[0]) and np.isnan(st[1])
        else:
            assert st[0] == want.min() and st[1] == want.max(), name
        # the same tallies from a device destination (whole rows only)
        if (lo, hi) == (0, N_ROWS):
            _, st2 = s.ctx.expr_eval(code, consts, _lib.GD_EX_TO_COLUMN, 2, stats=True)
            assert np.array_equal(st, st2, equal_nan=True)


def test_columns_weights_and_loglikes_leaves(weighted, unit):
    from getdist_amd.colexpr import col, loglikes, weights

    for s, X, w in (weighted, unit):
        wv = np.ones(len(X)) if w is None else w
        e = col(4)
        want = X[:, 4].copy()
        for j in range(5, 20):  # 16 distinct columns, 4 .. 19 (finite ones: a left-to-right sum)
            e, want = e + col(j), want + X[:, j]
        cases.same_bits(e.eval(s), want, "16 columns")
        with np.errstate(all="ignore"):
            cases.same_bits((col(0) * col(0) - col(0)).eval(s), X[:, 0] * X[:, 0] - X[:, 0], "the same column twice")
            cases.same_bits((weights * col(1) + weights).eval(s), wv * X[:, 1] + wv, "weights leaf")
        cases.same_bits(weights.eval(s), wv, "weights alone")
        # the loglikes leaf reads the last spare column, which the caller fills
        ll = np.random.default_rng(5).standard_normal(len(X)) ** 2
        s.loglikes = ll
        try:
            cases.same_bits((loglikes * 0.5 - col(5)).eval(s), ll * 0.5 - X[:, 5], "loglikes leaf")
        finally:
            s.loglikes = None


def test_two_runs_bit_identical(weighted):
    from getdist_amd import _lib

    s, X, _ = weighted
    code, consts = cases.code128(_leaves()).compile(s)
    a, sa = s.ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, stats=True)
    a = np.array(a)
    b, sb = s.ctx.expr_eval(code, consts, _lib.GD_EX_TO_HOST_F64, stats=True)
    assert np.array_equal(a.view(np.uint64), np.array(b).view(np.uint64)) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64))


def test_bad_arguments_return_before_a_launch(weighted):
    from getdist_amd import _lib
    from getdist_amd._lib import Context, GdhipError
    from getdist_amd.colexpr import OP

    s, _, _ = weighted
    ctx = s.ctx
    C, K, ADD, NEG, WH = OP["COL"], OP["CONST"], OP["ADD"], OP["NEG"], OP["WHERE"]
    F64, COLUMN = _lib.GD_EX_TO_HOST_F64, _lib.GD_EX_TO_COLUMN
    ok = [(C, 0)]

    def refused(code, consts=(), dst=F64, **kw):
        with pytest.raises(GdhipError) as e:
            ctx.expr_eval(np.array(code, dtype=np.int32).reshape(-1, 2), np.array(consts, dtype=float), dst, **kw)
        assert e.value.code == _lib.GD_ERR_BADARG
        return str(e.value)

    assert "underflow" in refused([(C, 0), (ADD, 0)]) and "underflow" in refused([(NEG, 0)])
    assert "underflow" in refused([(C, 0), (C, 1), (WH, 0)])
    assert "deeper" in refused([(C, 0)] * 17 + [(ADD, 0)] * 16)
    assert "exactly one" in refused([(C, 0), (C, 1)])
    assert "unknown op" in refused([(C, 0), (len(_lib.GD_EX_OPS), 0)]) and "unknown op" in refused([(-3, 0)])
    assert "column" in refused([(C, ctx.n + ctx.EXTRA_COLS)]) and "column" in refused([(C, -2)])
    assert "constant" in refused([(K, 0)]) and "constant" in refused([(K, 1)], [1.0])
    assert "constants" in refused(ok, np.zeros(33))
    assert "length" in refused([(C, 0)] + [(NEG, 0)] * 128) and "length" in refused(np.zeros((0, 2)))
    assert "distinct" in refused([(C, j) for j in range(17)] + [(ADD, 0)] * 16)
    assert "slot" in refused(ok, dst=COLUMN, dst_arg=ctx.EXTRA_COLS) and "slot" in refused(ok, dst=COLUMN, dst_arg=-1)
    assert "destination" in refused(ok, dst=4) and "destination" in refused(ok, dst=-1)
    for lo, hi in [(5, 5), (6, 5), (-1, 5), (0, ctx.N + 1)]:
        assert "row range" in refused(ok, lo=lo, hi=hi)
    assert "every row" in refused(ok, dst=COLUMN, lo=1) and "every row" in refused(ok, dst=_lib.GD_EX_TO_AUXW, hi=ctx.N - 1)
    # the context still works, and one without samples refuses
    assert ctx.expr_eval(np.array(ok, dtype=np.int32), np.zeros(0), F64, lo=0, hi=4).shape == (4,)
    empty = Context(0)
    try:
        with pytest.raises(GdhipError) as e:
            empty.expr_eval(np.array(ok, dtype=np.int32), np.zeros(0), F64, lo=0, hi=1)
        assert e.value.code == _lib.GD_ERR_BADARG and "no samples" in str(e.value)
    finally:
        empty.close()


# ---- the transcendental class ---------------------------------------------------------------------------------------------------
ULP_CAP = {"exp": 3, "log": 3, "log10": 3, "log2": 3, "sin": 4, "cos": 4, "tan": 5, "arctan": 5, "tanh": 5, "arctan2": 6,
           "power": 16}


def _max_ulp_error(name, x, y, values):
    """the largest |value - truth| in units of np.spacing(truth rounded to double); the truth and the difference are
    formed in extended precision (np.longdouble with a 63-bit mantissa, else mpmath at 113 bits)"""
    if np.finfo(np.longdouble).nmant >= 63:
        f = getattr(np, name)
        xl = x.astype(np.longdouble)
        truth = f(xl) if y is None else f(xl, y.astype(np.longdouble))
        unit_ = np.abs(np.spacing(truth.astype(np.float64))).astype(np.longdouble)
        return float(np.max(np.abs(values.astype(np.longdouble) - truth) / unit_))
    import mpmath

    mpmath.mp.prec = 113
    fn = {"arctan": mpmath.atan, "arctan2": mpmath.atan2, "power": mpmath.power}.get(name) or getattr(mpmath, name)
    worst = 0.0
    for k in range(len(x)):
        t = fn(mpmath.mpf(float(x[k]))) if y is None else fn(mpmath.mpf(float(x[k])), mpmath.mpf(float(y[k])))
        worst = max(worst, float(abs(mpmath.mpf(float(values[k])) - t) / mpmath.mpf(float(abs(np.spacing(float(t)))))))
    return worst


def test_transcendental_ops_within_the_opencl_bounds():
    from getdist_amd._lib import Context
    from getdist_amd.colexpr import col

    rng = np.random.default_rng(31)
    n = 20_011
    X = np.empty((n, 4), order="F")
    X[:, 0] = rng.uniform(-20, 20, n)                       # exp sin cos tan arctan tanh, first argument of arctan2
    X[:, 1] = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))  # the logarithms, base of pow
    X[:, 2] = rng.uniform(-3, 3, n)                         # exponent of pow, second argument of arctan2
    X[:, 3] = 0.0
    ctx = Context(0)
    try:
        ctx.upload(X)
        s = Bare(ctx)
        for name, cap in ULP_CAP.items():
            f = getattr(np, name)
            if name in ("log", "log10", "log2"):
                x, y, e = X[:, 1], None, f(col(1))
            elif name == "power":
                x, y, e = X[:, 1], X[:, 2], f(col(1), col(2))
            elif name == "arctan2":
                x, y, e = X[:, 0], X[:, 2], f(col(0), col(2))
            else:
                x, y, e = X[:, 0], None, f(col(0))
            dev = _max_ulp_error(name, x, y, e.eval(s))
            ref = _max_ulp_error(name, x, y, f(x) if y is None else f(x, y))
            print("%-8s device %.2f ulp   numpy %.2f ulp   cap %d" % (name, dev, ref, cap))
            assert dev <= cap, name
    finally:
        ctx.close()


# ---- end to end on an MCSamples -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mcs():
    from getdist_amd.mcsamples import MCSamples

    rng = np.random.default_rng(77)
    X = rng.standard_normal((N_ROWS, 6)) * np.array([1.0, 0.5, 2.0, 1.0, 3.0, 0.1]) + np.array([0.2, 0.0, 1.0, 0.0, -1.0, 5.0])
    X[1:, 0] = 0.7 * X[:-1, 0] + 0.3 * X[1:, 0]  # some autocorrelation
    w = rng.integers(1, 6, N_ROWS).astype(float)
    ll = 0.5 * np.sum((X - X.mean(axis=0)) ** 2, axis=1)
    mc = MCSamples(samples=X, weights=w, loglikes=ll, names=["a", "b", "c", "d", "x", "y"])
    yield mc
    mc.ctx.close()


def _exprs(p):
    return p.a * np.sqrt(abs(p.b) / 0.3) - p.c, (p.d > 0.1) & ~(p.a < -1), np.minimum(p.x, 0.0) * p.y + 1.0


def test_statistics_of_expressions_equal_those_of_their_host_vectors(mcs):
    from getdist_amd.colexpr import loglikes, weights

    mc = mcs
    e, m, e2 = _exprs(mc.getDeviceParams())
    ev, mv, e2v = e.eval(mc), m.eval(mc), e2.eval(mc)
    eh, mh, e2h = _exprs(mc.getParams())
    cases.same_bits(ev, eh, "e"), cases.same_bits(mv, mh, "m"), cases.same_bits(e2v, e2h, "e2")
    assert ev.flags.owndata and mv.dtype == bool and 1000 < mv.sum() < N_ROWS - 1000

    def same(x, y):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))

    same(mc.mean(e), mc.mean(ev)), same(mc.var(e), mc.var(ev)), same(mc.std(e), mc.std(ev))
    same(mc.cov([e, "a", e2]), mc.cov([ev, "a", e2v])), same(mc.corr([e, "a", e2]), mc.corr([ev, "a", e2v]))
    same(mc.mean([e, "b", e2]), mc.mean([ev, "b", e2v]))
    same(mc.weighted_sum(e), mc.weighted_sum(ev))
    same(mc.confidence(e, [0.16, 0.84]), mc.confidence(ev, [0.16, 0.84]))
    same(mc.confidence(e, 0.05, upper=True), mc.confidence(ev, 0.05, upper=True))
    same(mc.twoTailLimits(e, 0.95), mc.twoTailLimits(ev, 0.95))
    h = mc.initParamConfidenceData(e)
    assert h.vec is e
    same(mc.confidence(h, [0.16, 0.84]), mc.confidence(mc.initParamConfidenceData(ev), [0.16, 0.84]))
    same(mc.getAutocorrelation(e, maxOff=5), mc.getAutocorrelation(ev, maxOff=5))
    same(mc.getCorrelationLength(e), mc.getCorrelationLength(ev))
    same(mc.getEffectiveSamples(e), mc.getEffectiveSamples(ev))
    same(mc.mean_diff(e), mc.mean_diff(ev))
    same(mc.mean(e, where=m), mc.mean(ev, where=mv)), same(mc.var(e, where=m), mc.var(ev, where=mv))
    same(mc.std(e, where=m), mc.std(ev, where=mv))
    same(mc.mean("a", where=m), mc.mean("a", where=mv))
    same(mc.cov([e, "b"], where=m), mc.cov([ev, "b"], where=mv))
    same(mc.get_norm(where=m), mc.get_norm(where=mv))
    same(mc.weighted_sum(e, where=m), mc.weighted_sum(ev, where=mv))
    # the loglikes and weights leaves, as vectors and in a mask
    g, gm = loglikes * 0.5 + weights, (loglikes < 3.0) | (weights > 4)
    gv, gmv = g.eval(mc), gm.eval(mc)
    cases.same_bits(gv, mc.loglikes * 0.5 + mc.weights, "g"), cases.same_bits(gmv, (mc.loglikes < 3.0) | (mc.weights > 4), "gm")
    same(mc.mean(g), mc.mean(gv)), same(mc.cov([g, e, "c"], where=gm), mc.cov([gv, ev, "c"], where=gmv))
    same(mc.confidence(g, [0.5]), mc.confidence(gv, [0.5]))
    # nothing is left selected, and the base statistics are untouched
    same(mc.mean("a"), mc.means[0]), same(mc.get_norm(), mc.weights.sum())


def test_mutators_take_expressions(mcs):
    def state(mc):
        return mc.samples, mc.weights, mc.loglikes, mc.means, np.array(mc.numrows)

    def check(do_expr, do_host):
        x, y = mcs.copy(), mcs.copy()
        try:
            do_expr(x, x.getDeviceParams()), do_host(y, y.getParams())
            for u, v in zip(state(x), state(y)):
                cases.same_bits(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), "state")
            return x.numrows, x.n
        finally:
            x.ctx.close(), y.ctx.close()

    assert check(lambda s, p: s.addDerived(_exprs(p)[0], "e"), lambda s, p: s.addDerived(_exprs(p)[0], "e")) == (N_ROWS, 7)
    rw = lambda p: 0.5 * ((p.a - 0.2) / 0.7) ** 2  # noqa: E731
    assert check(lambda s, p: s.reweightAddingLogLikes(rw(p)), lambda s, p: s.reweightAddingLogLikes(rw(p)))[0] == N_ROWS
    kept = check(lambda s, p: s.filter(_exprs(p)[1]), lambda s, p: s.filter(_exprs(p)[1]))[0]
    assert 1000 < kept < N_ROWS - 1000


def test_one_expression_two_sample_sets_and_errors(mcs):
    from getdist_amd.chains import ParamError, WeightedSampleError
    from getdist_amd.colexpr import col, loglikes
    from getdist_amd.mcsamples import MCSamples

    rng = np.random.default_rng(78)
    Y = rng.standard_normal((513, 3))
    other = MCSamples(samples=Y, names=["c", "zz", "a"])  # the shared names sit in other columns; unit weights
    try:
        e = col("a") * 2.0 - abs(col("c"))
        cases.same_bits(e.eval(mcs), mcs.samples[:, 0] * 2.0 - abs(mcs.samples[:, 2]), "first set")
        cases.same_bits(e.eval(other), Y[:, 2] * 2.0 - abs(Y[:, 0]), "second set")
        assert other.mean(e) == other.mean(e.eval(other))
        with pytest.raises(WeightedSampleError, match="logLikes"):
            other.mean(loglikes + 1.0)
    finally:
        other.ctx.close()
    p = mcs.getDeviceParams()
    with pytest.raises(ParamError):
        mcs.mean(col("nope") * 2.0)
    with pytest.raises(WeightedSampleError, match="boolean"):
        mcs.mean("a", where=p.a * 2.0)
    with pytest.raises(WeightedSampleError, match="boolean"):
        mcs.get_norm(where=p.a)
    with pytest.raises(WeightedSampleError, match="vector arguments"):
        mcs.cov([p.a + float(k) for k in range(5)])
    with pytest.raises(WeightedSampleError, match="vector arguments"):
        mcs.cov([loglikes + float(k) for k in range(4)])
    assert mcs.cov([p.a + float(k) for k in range(4)]).shape == (4, 4)
    assert mcs.mean("a") == mcs.means[0]
