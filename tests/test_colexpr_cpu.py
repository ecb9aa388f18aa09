"""
CPU tests of column expressions (getdist_amd/colexpr.py): building and typing of the tree, compilation to the postfix
program of gd_expr_eval and its limits, and the interpreter step of csrc/colexpr.hpp -- the source the kernel compiles --
built with g++ and compared with numpy BIT FOR BIT on the exact class of ops.  The context double is the one of
fake_ctx.py with an ``expr_eval`` that runs that harness over its host columns.
"""

import ctypes
import os
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
import colexpr_cases as cases  # noqa: E402

PI32, PD = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def harness():
    return build_colexpr.load()


def _c_args(code, consts):
    code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 2)
    consts = np.ascontiguousarray(consts, dtype=np.float64).ravel()
    return code, consts, (code.ctypes.data_as(PI32), len(code), consts.ctypes.data_as(PD), consts.size)


class ExprContext(FakeContext):
    """fake_ctx.FakeContext plus Context.expr_eval, answered by the g++ build of csrc/colexpr.hpp"""

    lib = None

    def expr_eval(self, code, consts, dst, dst_arg=0, lo=0, hi=None, stats=False):
        code, consts, args = _c_args(code, consts)
        hi = self.N if hi is None else hi
        cols = np.asfortranarray(self.s)
        w = None if self.w is None else np.ascontiguousarray(self.w)
        out = np.empty(self.N)
        rc = self.lib.colexpr_run(*args, cols.shape[1], cols.ctypes.data_as(PD), None if w is None else w.ctypes.data_as(PD),
                                  self.N, out.ctypes.data_as(PD))
        if rc != 0:
            raise ValueError(self.lib.colexpr_check(*args, cols.shape[1]).decode())
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


NAMES = cases.NAMES


@pytest.fixture(scope="module")
def mc(harness):
    from getdist_amd.mcsamples import MCSamples

    ExprContext.lib = harness
    X, w, ll = cases.inputs()
    with np.errstate(all="ignore"):
        return MCSamples(samples=X, weights=w, loglikes=ll, names=NAMES, _context_factory=ExprContext)


class _Stub:
    """what compile() needs of a sample set"""

    def __init__(self, n):
        self.n = n
        self.ctx = FakeContext

    def _col(self, par):
        return par if isinstance(par, int) else NAMES.index(par)


def _ops(expr, samples=None):
    code, consts = expr.compile(samples or _Stub(4))
    return [(_lib.GD_EX_OPS[o], int(a)) for o, a in code], list(consts)


def test_python_constants_match_the_header():
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gdhip.h")).read()
    defs = {k: int(v.strip("()")) for k, v in re.findall(r"#define GD_EX_(\w+) (\(?-?\d+\)?)", text)}
    assert defs.pop("NUM_OPS") == len(_lib.GD_EX_OPS) == 34
    for k, name in enumerate(_lib.GD_EX_OPS):
        assert defs.pop(name) == k == OP[name], name
    for name in ("MAX_CODE", "MAX_STACK", "MAX_CONST", "MAX_COLS", "WEIGHT", "TO_COLUMN", "TO_AUXW", "TO_HOST_F64", "TO_HOST_U8"):
        assert defs.pop(name) == getattr(_lib, "GD_EX_" + name), name
    assert not defs
    assert (_lib.GD_EX_MAX_CODE, _lib.GD_EX_MAX_STACK, _lib.GD_EX_MAX_CONST, _lib.GD_EX_MAX_COLS) == (128, 16, 32, 16)


# ---- building and compiling ------------------------------------------------------------------------------------------------
def test_programs_op_for_op():
    a, b, c = col("a"), col("b"), col("c")
    assert _ops(a * np.sqrt(b / 0.3)) == ([("COL", 0), ("COL", 1), ("CONST", 0), ("DIV", 0), ("SQRT", 0), ("MUL", 0)], [0.3])
    ops, consts = _ops((c > 70) & ~(a < 0.3) | (2.0 - b == ce.weights))
    assert ops == [("COL", 2), ("CONST", 0), ("GT", 0), ("COL", 0), ("CONST", 1), ("LT", 0), ("NOT", 0), ("AND", 0),
                   ("CONST", 2), ("COL", 1), ("SUB", 0), ("COL", _lib.GD_EX_WEIGHT), ("EQ", 0), ("OR", 0)]
    assert consts == [70.0, 0.3, 2.0]
    # a constant met twice is stored once; the loglikes live in the last spare column; where pops c, a, b
    ops, consts = _ops(ce.where(a > 0.5, ce.loglikes + 0.5, -abs(col(3))))
    assert ops == [("COL", 0), ("CONST", 0), ("GT", 0), ("COL", 4 + 4 - 1), ("CONST", 0), ("ADD", 0), ("COL", 3), ("ABS", 0),
                   ("NEG", 0), ("WHERE", 0)]
    assert consts == [0.5]
    assert OP["COL"] == 0 and OP["WHERE"] == len(_lib.GD_EX_OPS) - 1


def test_operators_and_reflected_forms():
    a = col("a")
    for expr, kind, first in [(a + 1, "ADD", "col"), (1 + a, "ADD", "const"), (a - 1, "SUB", "col"), (1 - a, "SUB", "const"),
                              (a * 2, "MUL", "col"), (2 * a, "MUL", "const"), (a / 2, "DIV", "col"), (2 / a, "DIV", "const"),
                              (a ** 3, "POW", "col"), (3 ** a, "POW", "const"), (np.float64(2) * a, "MUL", "const"),
                              (np.array(2.0) - a, "SUB", "const"), (a < 1, "LT", "col"), (1 < a, "GT", "col"),
                              (a <= 1, "LE", "col"), (a >= 1, "GE", "col"), (a == 1, "EQ", "col"), (a != 1, "NE", "col")]:
        assert isinstance(expr, ColumnExpr) and expr.kind == kind and expr.args[0].kind == first, (kind, first)
    assert (-a).kind == "NEG" and abs(a).kind == "ABS" and (+a) is a
    m = a > 0
    assert (m & True).kind == "AND" and (True & m).kind == "AND" and (m | m).kind == "OR" and (~m).kind == "NOT"
    assert m.is_bool and (~m).is_bool and not (m + 1).is_bool and not (+m).is_bool and not (m * m).is_bool
    assert _ops(+m) == _ops(m)  # promotion to float costs no instruction


def test_every_ufunc_of_the_closed_set():
    a, b = col("a"), col("b")
    assert len(ce.UFUNCS) == 33
    for name in ce.UFUNCS:
        uf = getattr(np, name)
        e = uf(a) if uf.nin == 1 else uf(a, b)
        want = "pos" if name == "positive" else (ce._UNARY.get(name) or ce._BINARY[name])
        assert isinstance(e, ColumnExpr) and (e is a if name == "positive" else e.kind == want), name
        assert e.is_bool == (want in ce._BOOL_OPS), name
        if uf.nin == 2:
            assert uf(1.5, a).args[0].kind == "const" and uf(a, np.float32(2)).args[1].args == (2.0,)
    assert np.abs(a).kind == "ABS" and np.true_divide(a, b).kind == "DIV"
    assert np.power(a, 2).kind == "POW"  # only the ** operator takes numpy's scalar fast paths
    assert np.logical_and(a, b).is_bool  # the ufunc takes floats, the & operator does not


def test_unsupported_numpy_calls_raise():
    a = col("a")
    for fn, name in [(np.arcsin, "arcsin"), (np.floor, "floor"), (np.isnan, "isnan"), (np.hypot, "hypot")]:
        with pytest.raises(TypeError, match=name):
            fn(a) if fn.nin == 1 else fn(a, a)
    with pytest.raises(TypeError, match="out"):
        np.sqrt(a, out=np.zeros(3))
    with pytest.raises(TypeError, match="reduce"):
        np.add.reduce(a)
    with pytest.raises(TypeError, match="sum"):
        np.sum(a)
    for bad in (np.zeros(3), np.zeros((1,)), np.zeros((2, 2))):
        with pytest.raises(TypeError, match="host array"):
            a + bad
        with pytest.raises(TypeError, match="host array"):
            bad * a
        with pytest.raises(TypeError, match="host array"):
            np.maximum(a, bad)
    with pytest.raises(TypeError):
        a + "x"


def test_where_and_clip():
    a, b = col("a"), col("b")
    w = np.where(a > 0, a, 0.0)
    assert w.kind == "WHERE" and [x.kind for x in w.args] == ["GT", "col", "const"] and not w.is_bool
    assert np.where(a > 0, b > 0, True).is_bool
    assert _ops(ce.where(a, 1.0, b)) == ([("COL", 0), ("CONST", 0), ("COL", 1), ("WHERE", 0)], [1.0])
    c = np.clip(a, -1.0, b)
    assert _ops(c) == ([("COL", 0), ("CONST", 0), ("MAX", 0), ("COL", 1), ("MIN", 0)], [-1.0])
    assert _ops(np.clip(a, None, 2.0)) == ([("COL", 0), ("CONST", 0), ("MIN", 0)], [2.0])
    with pytest.raises(TypeError, match="out"):
        np.clip(a, 0, 1, out=np.zeros(3))


def test_scalar_power_rewrites():
    a = col("a")
    assert _ops(a ** 2)[0] == [("COL", 0), ("SQUARE", 0)] and _ops(a ** 2.0) == _ops(a ** np.int64(2))
    assert _ops(a ** 0.5)[0] == [("COL", 0), ("SQRT", 0)]
    assert _ops(a ** -1)[0] == [("COL", 0), ("RECIP", 0)]
    assert (a ** 1) is a and _ops((a > 0) ** 1) == _ops(a > 0) and not ((a > 0) ** 1).is_bool
    for e in (3, -2, 0, 1.5, -0.5):
        assert _ops(a ** e) == ([("COL", 0), ("CONST", 0), ("POW", 0)], [float(e)])
    assert _ops(a ** col("b"))[0][-1] == ("POW", 0) and _ops(2 ** a)[0] == [("CONST", 0), ("COL", 0), ("POW", 0)]


def test_typing_bool_hash_and_immutability():
    a = col("a")
    for f in (lambda: a & (a > 0), lambda: (a > 0) | a, lambda: ~a, lambda: a & 1, lambda: 1.0 | (a > 0)):
        with pytest.raises(TypeError):
            f()
    with pytest.raises(TypeError, match="truth value"):
        bool(a > 0)
    with pytest.raises(TypeError, match="truth value"):
        0 < a < 1
    with pytest.raises(TypeError):
        hash(a)
    with pytest.raises(TypeError):
        {a: 1}
    with pytest.raises(AttributeError):
        a.kind = "const"
    with pytest.raises(AttributeError):
        del a.args
    with pytest.raises(TypeError):
        col(1.5)


def _sum(leaves):
    out = leaves[0]
    for x in leaves[1:]:
        out = out + x
    return out


def _nest(leaves):
    """a0 + (a1 + (a2 + ...)): the stack gets as deep as there are leaves"""
    out = leaves[-1]
    for x in reversed(leaves[:-1]):
        out = x + out
    return out


def test_limits_one_below_and_one_above(harness):
    a = col("a")
    st = _Stub(40)

    def accepted(expr):
        code, consts = expr.compile(st)
        _, _, args = _c_args(code, consts)
        assert harness.colexpr_check(*args, 44) is None
        return len(code), harness.colexpr_depth(*args, 44), len(consts)

    # 128 instructions: 64 leaves + 63 adds + 1 negation
    assert accepted(-_sum([a] * 64))[0] == _lib.GD_EX_MAX_CODE == 128
    assert accepted(_sum([a] * 64))[0] == 127
    with pytest.raises(ValueError, match="instructions"):
        (-(-_sum([a] * 64))).compile(st)
    # stack depth 16
    assert accepted(_nest([a] * 16))[1] == _lib.GD_EX_MAX_STACK == 16 and accepted(_nest([a] * 15))[1] == 15
    with pytest.raises(ValueError, match="stack"):
        _nest([a] * 17).compile(st)
    # 32 distinct constants
    assert accepted(_sum([a] + [float(k) for k in range(32)]))[2] == _lib.GD_EX_MAX_CONST == 32
    assert accepted(_sum([a] + [float(k) for k in range(31)]))[2] == 31
    assert accepted(_sum([a] + [float(k % 32) for k in range(40)]))[2] == 32  # repeats share a slot
    with pytest.raises(ValueError, match="constants"):
        _sum([a] + [float(k) for k in range(33)]).compile(st)
    # 16 distinct columns (the weights count)
    accepted(_sum([col(j) for j in range(16)]))
    accepted(_sum([col(j) for j in range(15)] + [ce.weights, col(3), col(7)]))
    with pytest.raises(ValueError, match="columns"):
        _sum([col(j) for j in range(17)]).compile(st)
    with pytest.raises(ValueError, match="columns"):
        _sum([col(j) for j in range(16)] + [ce.weights]).compile(st)


def test_native_check_refuses_what_the_entry_point_must(harness):
    """ex_pack is the validation gd_expr_eval runs before any launch"""
    C, K, ADD, WH = OP["COL"], OP["CONST"], OP["ADD"], OP["WHERE"]

    def check(code, consts=(), ncols=8):
        _, _, args = _c_args(np.array(code, dtype=np.int32), np.array(consts, dtype=float))
        return harness.colexpr_check(*args, ncols)

    assert check([(C, 0)]) is None and check([(C, 7)]) is None and check([(C, -1)]) is None
    assert check([(K, 0), (C, 1), (C, 2), (WH, 0)], [1.0]) is None
    assert b"underflow" in check([(C, 0), (ADD, 0)])
    assert b"underflow" in check([(OP["NEG"], 0)])
    assert b"underflow" in check([(C, 0), (C, 1), (WH, 0)])
    assert b"exactly one" in check([(C, 0), (C, 1)])
    assert b"unknown op" in check([(C, 0), (len(_lib.GD_EX_OPS), 0)]) and b"unknown op" in check([(-1, 0)])
    assert b"column" in check([(C, 8)]) and b"column" in check([(C, -2)])
    assert b"constant" in check([(K, 0)]) and b"constant" in check([(K, 1)], [1.0]) and b"constant" in check([(K, -1)], [1.0])
    assert b"deeper" in check([(C, 0)] * 17 + [(ADD, 0)] * 16)
    assert check([(C, 0)] * 16 + [(ADD, 0)] * 15) is None
    assert b"length" in check([(C, 0)] + [(OP["NEG"], 0)] * 128)
    assert check([(C, 0)] + [(OP["NEG"], 0)] * 127) is None
    assert b"distinct" in check([(C, j) for j in range(17)] + [(ADD, 0)] * 16, ncols=20)
    _, _, args = _c_args(np.zeros((0, 2), dtype=np.int32), np.zeros(0))
    assert b"length" in harness.colexpr_check(*args, 8)


# ---- the interpreter step against numpy, bit for bit --------------------------------------------------------------------------
_same_bits, EXACT = cases.same_bits, cases.EXACT


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_ops_bit_equal_to_numpy(mc, name):
    with np.errstate(all="ignore"):
        want = EXACT[name](mc.getParams())
    expr = EXACT[name](mc.getDeviceParams())
    assert isinstance(expr, ColumnExpr) and expr.is_bool == (want.dtype == bool)
    _same_bits(expr.eval(mc), want, name)


def test_leaves_weights_loglikes_and_index(mc):
    with np.errstate(all="ignore"):
        _same_bits((ce.weights * col(1) - ce.loglikes).eval(mc), mc.weights * mc.samples[:, 1] - mc.loglikes, "leaves")
    _same_bits(ce.weights.eval(mc), mc.weights, "weights")
    _same_bits(col("c").eval(mc), mc.samples[:, 2], "column")


def test_composites_at_the_limits(mc, harness):
    p, h = mc.getDeviceParams(), mc.getParams()
    e = cases.depth16(p)
    code, consts = e.compile(mc)
    _, _, args = _c_args(code, consts)
    assert harness.colexpr_depth(*args, 8) == 16
    with np.errstate(all="ignore"):
        _same_bits(e.eval(mc), cases.depth16(h), "depth 16")
    e = cases.code128(p)
    assert len(e.compile(mc)[0]) == 128
    with np.errstate(all="ignore"):
        _same_bits(e.eval(mc), cases.code128(h), "128 instructions")


# ---- getDeviceParams and the places that accept an expression (host logic, on the context double) --------------------------------
def test_device_params_layout_equals_get_params(harness):
    from getdist_amd.chains import ParSamples
    from getdist_amd.mcsamples import MCSamples

    ExprContext.lib = harness
    s = np.random.default_rng(5).standard_normal((40, 5))
    for names in (["aa", "aa.bb", "plain", "m.n.o", "aa.cc.dd"], ["aa.bb", "aa", "x", "y.z", "y"]):
        m = MCSamples(samples=s, names=names, _context_factory=ExprContext)
        before = m.getParams()

        def walk(host, dev, path):
            assert isinstance(dev, ParSamples) and sorted(vars(host)) == sorted(vars(dev)), path
            for k, v in vars(host).items():
                d = getattr(dev, k)
                if isinstance(v, ParSamples):
                    walk(v, d, path + k + ".")
                else:
                    name = (path + k)[:-len(".value")] if k == "value" and (path + k)[:-len(".value")] in names else path + k
                    assert isinstance(d, ColumnExpr) and d.kind == "col" and d.args == (name,), path + k
                    assert np.array_equal(d.eval(m), v), path + k

        walk(before, m.getDeviceParams(), "")
        after = m.getParams()  # getParams keeps handing out host vectors
        assert isinstance(after.plain if "plain" in names else after.x, np.ndarray)


@pytest.fixture(scope="module")
def mcfin(harness):
    """finite values only: a masked-out NaN still poisons a weighted sum (0 * NaN), on the host route as well"""
    from getdist_amd.mcsamples import MCSamples

    ExprContext.lib = harness
    rng = np.random.default_rng(11)
    X = rng.standard_normal((997, 4))
    return MCSamples(samples=X, weights=rng.integers(1, 5, len(X)).astype(float), loglikes=rng.standard_normal(len(X)) ** 2,
                     names=NAMES, _context_factory=ExprContext)


def test_expressions_where_host_vectors_are_accepted(mcfin):
    from getdist_amd.chains import ParamError, WeightedSampleError

    mc = mcfin
    p = mc.getDeviceParams()
    e = p.d * np.sqrt(abs(p.b) / 0.3) - np.minimum(p.d, 2.0)
    e2 = ce.loglikes * 0.5 + ce.weights
    both = (p.d > 0.0) & ~(p.b < -1)
    ev, e2v, mv = e.eval(mc), e2.eval(mc), both.eval(mc)
    assert mv.dtype == bool and 100 < mv.sum() < len(mv) - 100
    _same_bits(mv, (mc.samples[:, 3] > 0.0) & ~(mc.samples[:, 1] < -1), "mask")
    assert mc.mean(e, where=both) == mc.mean(ev, where=mv) and mc.var(e, where=both) == mc.var(ev, where=mv)
    assert np.array_equal(mc.cov([e, "d", e2], where=both), mc.cov([ev, "d", e2v], where=mv))
    assert mc.get_norm(where=both) == mc.get_norm(where=mv) == mc.weights[mv].sum()
    assert np.array_equal(mc.mean([e2, "d"]), mc.mean([e2v, "d"])) and mc.std(e2) == mc.std(e2v)
    assert mc.weighted_sum(e2) == mc.weighted_sum(e2v)
    assert np.array_equal(mc.confidence(e2, [0.16, 0.84]), mc.confidence(e2v, [0.16, 0.84]))
    h = mc.initParamConfidenceData(e2)
    assert h.vec is e2 and mc.confidence(h, 0.5) == mc.confidence(e2v, 0.5)
    assert np.array_equal(mc.mean_diff(e2), mc.mean_diff(e2v))
    with pytest.raises(WeightedSampleError, match="boolean"):
        mc.mean("a", where=e)
    with pytest.raises(ParamError):
        mc.mean(col("nope") + 1)
    with pytest.raises(WeightedSampleError, match="vector arguments"):
        mc.cov([e2 + k for k in range(5)])
    with pytest.raises(WeightedSampleError, match="vector arguments"):
        mc.cov([e2 + k for k in range(4)])  # the loglikes take the last spare column
    mc.cov([p.d + k for k in range(4)])
    share = mc._column_share
    try:
        mc._column_share = object()
        from getdist_amd.chains import MCSamplesError

        with pytest.raises(MCSamplesError, match="share of the columns"):
            e.eval(mc)
    finally:
        mc._column_share = share


def test_one_expression_on_two_sample_sets_and_renames(mc, harness):
    from getdist_amd.mcsamples import MCSamples

    ExprContext.lib = harness
    rng = np.random.default_rng(3)
    s = rng.standard_normal((50, 3))
    other = MCSamples(samples=s, names=["d", "zz", "a"], _context_factory=ExprContext)  # other order, no weights
    e = col("a") * 2.0 - col("d") * ce.weights
    with np.errstate(all="ignore"):
        _same_bits(e.eval(mc), mc.samples[:, 0] * 2.0 - mc.samples[:, 3] * mc.weights, "first")
    _same_bits(e.eval(other), s[:, 2] * 2.0 - s[:, 0] * 1.0, "second")


def test_an_error_after_the_mask_leaves_no_stale_like_weights(mcfin):
    """The mask of where= is written into the buffer the mean-likelihood weights live in: the claim on that buffer
    (_like_mode) is dropped before the write, so that an error raised while the columns are resolved cannot leave a later
    mean-likelihood density binning with weight * mask."""
    from getdist_amd.chains import ParamError, WeightedSampleError

    mc = mcfin
    p = mc.getDeviceParams()
    e, m = p.a * 2.0, p.d > 0.0
    for call, err in [(lambda: mc.cov([e, "nope"], where=m), ParamError),
                      (lambda: mc.cov([e + float(k) for k in range(5)], where=m), WeightedSampleError),
                      (lambda: mc.mean([e, "nope"], where=m), ParamError),
                      (lambda: mc.mean(np.zeros(3), where=m), WeightedSampleError)]:
        mc._like_mode = 0
        with pytest.raises(err):
            call()
        assert mc._like_mode is None and mc.ctx._w_sel == 0
    mc._like_mode = 1
    mc.get_norm(where=m)
    assert mc._like_mode is None and mc.ctx._w_sel == 0


def test_expressions_copy_and_pickle(mcfin):
    import copy
    import pickle

    e = col("a") * np.sqrt(abs(col("b")) / 0.3) - ce.loglikes
    m = (col("d") > 0.0) & ~(col("a") < -1)
    assert copy.copy(e) is e and copy.deepcopy(e) is e
    for x in (e, m, ce.weights):
        y = pickle.loads(pickle.dumps(x))
        assert isinstance(y, ColumnExpr) and y is not x and repr(y) == repr(x) and y.is_bool == x.is_bool
        _same_bits(y.eval(mcfin), x.eval(mcfin), "pickled")
    h = mcfin.initParamConfidenceData(e)
    h2 = copy.deepcopy(h)
    assert h2 is not h and h2.vec is e and mcfin.confidence(h2, 0.5) == mcfin.confidence(h, 0.5)


def test_expressions_and_masks_are_evaluated_once(mcfin):
    """getAutocorrelation / getCorrelationLength place the expression in its column once and take mean and variance from
    that column; a list under where= evaluates the mask once.  Same values as the host-vector route."""
    mc = mcfin
    p = mc.getDeviceParams()
    e, e2, m = p.a * 2.0 - p.b, abs(p.c) + 1.0, p.d > 0.0
    ev, e2v, mv = e.eval(mc), e2.eval(mc), m.eval(mc)
    calls = []
    real = mc.ctx.expr_eval
    mc.ctx.expr_eval = lambda *a, **k: (calls.append(a[2]), real(*a, **k))[1]
    try:
        got = mc.getAutocorrelation(e, maxOff=4)
        assert calls == [_lib.GD_EX_TO_COLUMN]
        del calls[:]
        length = mc.getCorrelationLength(e)
        assert calls == [_lib.GD_EX_TO_COLUMN]
        del calls[:]
        means = mc.mean([e, "b", e2], where=m)
        assert calls == [_lib.GD_EX_TO_AUXW, _lib.GD_EX_TO_COLUMN, _lib.GD_EX_TO_COLUMN]
    finally:
        del mc.ctx.expr_eval
    assert np.array_equal(got, mc.getAutocorrelation(ev, maxOff=4)) and length == mc.getCorrelationLength(ev)
    assert np.array_equal(mc.getAutocorrelation(e, maxOff=4, normalized=False), mc.getAutocorrelation(ev, maxOff=4, normalized=False))
    assert np.array_equal(means, mc.mean([ev, "b", e2v], where=mv))
