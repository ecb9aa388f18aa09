"""
Lazy expressions over the named columns of a device-resident sample set: the derived vector of the GetDist idiom

    p = samples.getDeviceParams()
    S8 = p.sigma8 * np.sqrt(p.omegam / 0.3)
    samples.mean(S8, where=p.H0 > 70)
    samples.confidence(S8, 0.95, upper=True)
    samples.addDerived(S8, name="S8")

evaluated in one fused pass on the device (gd_expr_eval, csrc/colexpr.hip) instead of one numpy temporary per operator and
an N-vector over PCIe.  Not in the reference, whose ``getParams()`` hands out host columns (that route is unchanged).

A :class:`ColumnExpr` is an immutable tree.  Its leaves are ``col(name_or_index)``, the specials ``loglikes`` and
``weights`` (the reference's -1 / -2 of ``_makeParamvec``) and float constants; a leaf refers to a parameter by NAME and is
looked up (``samples._col``) only when the expression is evaluated, so one expression can be applied to several sample
sets and survives renames.  Python operators, the numpy ufuncs of ``UFUNCS``, ``np.where`` and ``np.clip`` build nodes;
anything else raises TypeError.  Whether a node is boolean is tracked here (comparisons and logic are, the rest is float;
a boolean used in arithmetic counts as 0.0 / 1.0); on the device every value is a double.  That promotion DIFFERS from
numpy where every operand is boolean: for two masks ``m1 + m2`` and ``m1 * m2`` are the floats 0.0 / 1.0 / 2.0 here
(numpy keeps bool: True + True is True), and ``-m``, ``m1 - m2`` and ``abs(m)`` are accepted as floats where numpy raises
or keeps bool -- so ``addDerived(m1 + m2)`` counts the masks that hold, which the host idiom does not.  Write ``m1 | m2``
and ``m1 & m2`` for numpy's results.

``+ - * /``, ``sqrt``, ``square``, ``reciprocal``, ``negative``, ``absolute``, ``minimum``, ``maximum``, comparisons, logic and
``where`` give numpy's values bit for bit; ``x ** 2``, ``x ** 0.5``, ``x ** -1`` and ``x ** 1`` with a SCALAR exponent follow
numpy's fast paths (x * x, sqrt, 1 / x, x) and are exact too, every other power is the device library's ``pow``, as are
the other transcendental functions.  Division by zero and invalid operands give inf / NaN silently: numpy's
RuntimeWarning is not reproduced (the device has no warning channel).

Tabulated functions are nodes too (gd_expr_eval_tab): ``np.interp(expr, xp, fp, left, right)`` (or :func:`interp`),
``Density1D.Prob(expr, derivative)`` and ``Density2D.Prob(ex, ey)`` of densities.py.  Their tables -- a :class:`Table`, held
by the node and sent with every launch -- are host arrays; the values are numpy's ``np.interp``, this package's
``Density1D.Prob`` of the host vector and scipy's ``RectBivariateSpline.ev`` bit for bit.
"""

import numpy as np

from ._lib import (GD_EX_MAX_CODE, GD_EX_MAX_COLS, GD_EX_MAX_CONST, GD_EX_MAX_STACK, GD_EX_OPS, GD_EX_TO_AUXW, GD_EX_TO_COLUMN,
                   GD_EX_TO_HOST_F64, GD_EX_TO_HOST_U8, GD_EX_WEIGHT, GD_TAB_MAX_DOUBLES, GD_TAB_MAX_TABLES, GD_TAB_OPS)

OP = {name: k for k, name in enumerate(GD_EX_OPS)}

_UNARY = {"negative": "NEG", "absolute": "ABS", "sqrt": "SQRT", "square": "SQUARE", "reciprocal": "RECIP", "exp": "EXP",
          "log": "LOG", "log10": "LOG10", "log2": "LOG2", "sin": "SIN", "cos": "COS", "tan": "TAN", "arctan": "ATAN",
          "tanh": "TANH", "logical_not": "NOT"}
_BINARY = {"add": "ADD", "subtract": "SUB", "multiply": "MUL", "divide": "DIV", "true_divide": "DIV", "power": "POW",
           "arctan2": "ATAN2", "minimum": "MIN", "maximum": "MAX", "less": "LT", "less_equal": "LE", "greater": "GT",
           "greater_equal": "GE", "equal": "EQ", "not_equal": "NE", "logical_and": "AND", "logical_or": "OR"}
_BOOL_OPS = {"NOT", "LT", "LE", "GT", "GE", "EQ", "NE", "AND", "OR"}
UFUNCS = tuple(sorted(set(_UNARY) | set(_BINARY) | {"positive"}))  # the closed set __array_ufunc__ accepts


def _wrap(x):
    """An operand as a node: expressions as they are; Python and numpy scalars and 0-d arrays become constants."""
    if isinstance(x, ColumnExpr):
        return x
    if isinstance(x, (bool, np.bool_)):
        return ColumnExpr("const", (float(x),), True)
    if isinstance(x, (int, float, np.integer, np.floating)):
        return ColumnExpr("const", (float(x),), False)
    if isinstance(x, np.ndarray) and x.ndim == 0 and x.dtype.kind in "biuf":
        return ColumnExpr("const", (float(x),), x.dtype.kind == "b")
    if isinstance(x, np.ndarray):
        raise TypeError("a host array of shape %s cannot be mixed into a device column expression (only scalars can)"
                        % (x.shape,))
    raise TypeError("unsupported operand for a column expression: %s" % type(x).__name__)


class Table:
    """The payload of a look-up node: ``kind`` ("INTERP", "SPLINE1" or "SPLINE2", an op of gd_expr_eval_tab), its host
    ``arrays`` (float64, C-contiguous, read-only copies: knots and values / knots and interval coefficients / tx, ty, c),
    the sizes ``nx`` and ``ny`` gd_expr_table wants, ``left`` / ``right`` of np.interp and the derivative order ``deriv`` of
    a 1D spline.  Immutable; two nodes that hold the SAME Table object share one slot of a program."""

    __slots__ = ("kind", "arrays", "nx", "ny", "left", "right", "deriv")

    def __init__(self, kind, arrays, nx, ny=0, left=0.0, right=0.0, deriv=0):
        frozen = []
        for a in arrays:
            a = np.array(a, dtype=np.float64, order="C", copy=True)
            a.flags.writeable = False
            frozen.append(a)
        for k, v in zip(self.__slots__, (kind, tuple(frozen), int(nx), int(ny), float(left), float(right), int(deriv))):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("Table is immutable")

    def __delattr__(self, name):
        raise AttributeError("Table is immutable")

    def __reduce__(self):
        return Table, (self.kind, self.arrays, self.nx, self.ny, self.left, self.right, self.deriv)

    @property
    def doubles(self):
        return sum(a.size for a in self.arrays)

    def __repr__(self):
        shape = "%d" % self.nx if self.kind != "SPLINE2" else "%dx%d" % (self.nx - 4, self.ny - 4)
        return "<%s table %s>" % (self.kind.lower(), shape)


def _is_scalar(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_))


class ColumnExpr:
    """One node of an expression tree: ``kind`` is "col", "loglikes", "weights", "const", "pos" (promotion to float, no
    instruction) or an op name of gd_expr_eval; ``args`` its operands; ``is_bool`` the type tracked on the host.  A look-up
    node (kind "INTERP", "SPLINE1" or "SPLINE2", an op of gd_expr_eval_tab) holds its :class:`Table` behind its operands."""

    __slots__ = ("kind", "args", "is_bool")
    __array_priority__ = 1000
    __hash__ = None  # == builds a node

    def __init__(self, kind, args=(), is_bool=False):
        object.__setattr__(self, "kind", kind)
        object.__setattr__(self, "args", tuple(args))
        object.__setattr__(self, "is_bool", bool(is_bool))

    def __setattr__(self, name, value):
        raise AttributeError("ColumnExpr is immutable")

    def __delattr__(self, name):
        raise AttributeError("ColumnExpr is immutable")

    def __reduce__(self):  # pickle (a handle or a user object holding an expression goes to a worker)
        return ColumnExpr, (self.kind, self.args, self.is_bool)

    def __copy__(self):  # immutable: a copy is the object itself
        return self

    def __deepcopy__(self, memo):
        return self

    def __bool__(self):
        raise TypeError("the truth value of a column expression is not defined: combine comparisons with & and | "
                        "(a < x < b is written (a < x) & (x < b))")

    def __repr__(self):
        if self.kind == "col":
            return "col(%r)" % (self.args[0],)
        if self.kind in ("loglikes", "weights"):
            return self.kind
        if self.kind == "const":
            return repr(self.args[0])
        return "%s(%s)" % (self.kind.lower(), ", ".join(repr(a) for a in self.args))  # (a Table names its kind and shape)

    # ---- node builders
    @staticmethod
    def _unary(op, a):
        return ColumnExpr(op, (_wrap(a),), op in _BOOL_OPS)

    @staticmethod
    def _binary(op, a, b):
        return ColumnExpr(op, (_wrap(a), _wrap(b)), op in _BOOL_OPS)

    def _logic(self, op, sym, a, b):
        a, b = _wrap(a), _wrap(b)
        if not (a.is_bool and b.is_bool):
            raise TypeError("%s needs boolean operands (comparisons); for float expressions use np.logical_%s"
                            % (sym, op.lower()))
        return ColumnExpr(op, (a, b), True)

    def _power(self, exponent):
        if _is_scalar(exponent):  # numpy's fast paths for a scalar exponent (bit-equal on numpy 2.2)
            if exponent == 2:
                return ColumnExpr._unary("SQUARE", self)
            if exponent == 0.5:
                return ColumnExpr._unary("SQRT", self)
            if exponent == -1:
                return ColumnExpr._unary("RECIP", self)
            if exponent == 1:
                return +self
        return ColumnExpr._binary("POW", self, exponent)

    # ---- arithmetic
    def __add__(self, o): return ColumnExpr._binary("ADD", self, o)
    def __radd__(self, o): return ColumnExpr._binary("ADD", o, self)
    def __sub__(self, o): return ColumnExpr._binary("SUB", self, o)
    def __rsub__(self, o): return ColumnExpr._binary("SUB", o, self)
    def __mul__(self, o): return ColumnExpr._binary("MUL", self, o)
    def __rmul__(self, o): return ColumnExpr._binary("MUL", o, self)
    def __truediv__(self, o): return ColumnExpr._binary("DIV", self, o)
    def __rtruediv__(self, o): return ColumnExpr._binary("DIV", o, self)
    def __pow__(self, o): return self._power(o)
    def __rpow__(self, o): return ColumnExpr._binary("POW", o, self)
    def __neg__(self): return ColumnExpr._unary("NEG", self)
    def __pos__(self): return ColumnExpr("pos", (self,), False) if self.is_bool else self
    def __abs__(self): return ColumnExpr._unary("ABS", self)

    # ---- comparisons
    def __lt__(self, o): return ColumnExpr._binary("LT", self, o)
    def __le__(self, o): return ColumnExpr._binary("LE", self, o)
    def __gt__(self, o): return ColumnExpr._binary("GT", self, o)
    def __ge__(self, o): return ColumnExpr._binary("GE", self, o)
    def __eq__(self, o): return ColumnExpr._binary("EQ", self, o)
    def __ne__(self, o): return ColumnExpr._binary("NE", self, o)

    # ---- logic (booleans only, as numpy's & | ~ refuse floats)
    def __and__(self, o): return self._logic("AND", "&", self, o)
    def __rand__(self, o): return self._logic("AND", "&", o, self)
    def __or__(self, o): return self._logic("OR", "|", self, o)
    def __ror__(self, o): return self._logic("OR", "|", o, self)

    def __invert__(self):
        if not self.is_bool:
            raise TypeError("~ needs a boolean operand (a comparison); for float expressions use np.logical_not")
        return ColumnExpr._unary("NOT", self)

    # ---- numpy
    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        name = ufunc.__name__
        if method != "__call__" or kwargs:
            raise TypeError("np.%s: only plain calls of a ufunc are supported on column expressions (no %s)"
                            % (name, method if method != "__call__" else ", ".join(sorted(kwargs)) + "="))
        if name == "positive" and len(inputs) == 1:
            return +_wrap(inputs[0])
        if name in _UNARY and len(inputs) == 1:
            return ColumnExpr._unary(_UNARY[name], inputs[0])
        if name in _BINARY and len(inputs) == 2:
            return ColumnExpr._binary(_BINARY[name], inputs[0], inputs[1])
        raise TypeError("np.%s is not supported on column expressions (supported: %s)" % (name, ", ".join(UFUNCS)))

    def __array_function__(self, func, types, args, kwargs):
        if func is np.where and len(args) == 3 and not kwargs:
            return where(*args)
        if func is np.clip:
            return _clip(*args, **kwargs)
        if func is np.interp:
            return interp(*args, **kwargs)
        raise TypeError("np.%s is not supported on column expressions" % getattr(func, "__name__", func))

    # ---- compilation and evaluation
    def uses_loglikes(self):
        return self.kind == "loglikes" or any(a.uses_loglikes() for a in self.args if isinstance(a, ColumnExpr))

    def compile(self, samples):
        """The postfix program (code, consts) of gd_expr_eval for ``samples``: ``code`` an (ncode, 2) int32 array of
        (op, arg), ``consts`` the float64 constants.  Names are resolved here (an unknown one raises ParamError); shared
        sub-trees are emitted once per use.  Raises ValueError when the program exceeds GD_EX_MAX_CODE instructions,
        GD_EX_MAX_STACK stack entries, GD_EX_MAX_CONST distinct constants or GD_EX_MAX_COLS distinct columns (the weights
        and the loglikes count as columns) -- and for an expression with table look-ups, whose program is a triple: see
        :meth:`compile_with_tables`."""
        code, consts, tables = self.compile_with_tables(samples)
        if tables:
            raise ValueError("the expression holds %d table look-up(s) (np.interp, Density.Prob): its program comes with "
                             "tables, use compile_with_tables(samples)" % len(tables))
        return code, consts

    def compile_with_tables(self, samples):
        """(code, consts, tables): :meth:`compile` for any expression.  ``tables`` lists the distinct :class:`Table`
        objects of the look-up nodes; the argument of a look-up op (_lib.GD_TAB_OPS) is its table's position there.  Also
        raises ValueError for more than GD_TAB_MAX_TABLES distinct tables and for a table of more than GD_TAB_MAX_DOUBLES
        doubles."""
        code, consts, cols, tables = [], {}, set(), []
        depth = [0, 0]  # current, deepest

        def push():
            depth[0] += 1
            depth[1] = max(depth[1], depth[0])

        def emit(node):
            k = node.kind
            if k in ("col", "loglikes", "weights"):
                if k == "col":
                    j = samples._col(node.args[0])
                else:
                    j = GD_EX_WEIGHT if k == "weights" else samples.n + samples.ctx.EXTRA_COLS - 1
                cols.add(j)
                code.append((OP["COL"], j))
                push()
            elif k == "const":
                key = np.float64(node.args[0]).tobytes()
                code.append((OP["CONST"], consts.setdefault(key, len(consts))))
                push()
            elif k == "pos":
                emit(node.args[0])
            elif k in GD_TAB_OPS:  # args: the operands, then the Table
                for a in node.args[:-1]:
                    emit(a)
                table = node.args[-1]
                slot = next((i for i, t in enumerate(tables) if t is table), len(tables))
                if slot == len(tables):
                    tables.append(table)
                code.append((GD_TAB_OPS[k], slot))
                depth[0] -= len(node.args) - 2
            else:
                for a in node.args:
                    emit(a)
                code.append((OP[k], 0))
                depth[0] -= len(node.args) - 1

        emit(self)
        if len(code) > GD_EX_MAX_CODE:
            raise ValueError("the expression compiles to %d instructions (at most %d)" % (len(code), GD_EX_MAX_CODE))
        if depth[1] > GD_EX_MAX_STACK:
            raise ValueError("the expression needs a stack of %d entries (at most %d)" % (depth[1], GD_EX_MAX_STACK))
        if len(consts) > GD_EX_MAX_CONST:
            raise ValueError("the expression has %d distinct constants (at most %d)" % (len(consts), GD_EX_MAX_CONST))
        if len(cols) > GD_EX_MAX_COLS:
            raise ValueError("the expression reads %d distinct columns (at most %d)" % (len(cols), GD_EX_MAX_COLS))
        if len(tables) > GD_TAB_MAX_TABLES:
            raise ValueError("the expression refers to %d distinct tables (at most %d)" % (len(tables), GD_TAB_MAX_TABLES))
        for t in tables:
            if t.doubles > GD_TAB_MAX_DOUBLES:
                raise ValueError("%r holds %d doubles (at most %d)" % (t, t.doubles, GD_TAB_MAX_DOUBLES))
        return (np.array(code, dtype=np.int32).reshape(-1, 2),
                np.frombuffer(b"".join(consts), dtype=np.float64).copy() if consts else np.zeros(0), tables)

    def _run(self, samples, dst, dst_arg=0):
        """Compile for ``samples``, make the loglikes resident when the expression reads them, and launch."""
        from .chains import MCSamplesError, WeightedSampleError

        if getattr(samples, "_column_share", None) is not None:
            raise MCSamplesError("column expressions need every column resident on one device: this context holds only "
                                 "its rank's share of the columns (multi-GPU expressions are not supported)")
        code, consts, tables = self.compile_with_tables(samples)
        if self.uses_loglikes():
            if samples.loglikes is None:
                raise WeightedSampleError("Samples do not have logLikes (expression reads loglikes)")
            samples.ctx.set_extra_column(samples.ctx.EXTRA_COLS - 1, samples.loglikes)
        if tables:
            return samples.ctx.expr_eval(code, consts, dst, dst_arg, tables=tables)
        return samples.ctx.expr_eval(code, consts, dst, dst_arg)

    def eval(self, samples):
        """The expression's value at every row of ``samples`` as an owned host array: float64, or bool for a boolean
        expression (fetched as one byte per row)."""
        if self.is_bool:
            return np.array(self._run(samples, GD_EX_TO_HOST_U8), dtype=bool)
        return np.array(self._run(samples, GD_EX_TO_HOST_F64), dtype=np.float64)

    def to_column(self, samples, slot):
        """Evaluate into spare column ``slot`` of the samples' context; returns the column index it is addressed by."""
        return self._run(samples, GD_EX_TO_COLUMN, slot)

    def to_aux_weights(self, samples):
        """Evaluate sample weight * value into the context's auxiliary weight buffer (what ``where=`` selects)."""
        self._run(samples, GD_EX_TO_AUXW)


def col(name_or_index):
    """The leaf for a parameter, by name (looked up when the expression is evaluated) or column index."""
    if isinstance(name_or_index, ColumnExpr):
        return name_or_index
    if not isinstance(name_or_index, (str, int, np.integer)) or isinstance(name_or_index, bool):
        name = getattr(name_or_index, "name", None)  # a ParamInfo
        if not isinstance(name, str):
            raise TypeError("col() takes a parameter name or a column index")
        name_or_index = name
    return ColumnExpr("col", (name_or_index if isinstance(name_or_index, str) else int(name_or_index),))


loglikes = ColumnExpr("loglikes")
weights = ColumnExpr("weights")


def where(c, a, b):
    """``a`` where ``c`` is non-zero, else ``b`` (np.where of three arguments); boolean when both branches are."""
    c, a, b = _wrap(c), _wrap(a), _wrap(b)
    return ColumnExpr("WHERE", (c, a, b), a.is_bool and b.is_bool)


def lookup(kind, table, *operands):
    """The float node that applies ``table`` (a :class:`Table` of that ``kind``) to its operand expression(s)."""
    return ColumnExpr(kind, tuple(_wrap(a) for a in operands) + (table,), False)


def interp(x, xp, fp, left=None, right=None, period=None):
    """``np.interp(x, xp, fp, left, right)`` of the expression ``x``: numpy's values bit for bit (``left`` / ``right``,
    NaN in gives NaN out, x equal to a knot gives its ``fp`` without arithmetic, repeated knots pick the last).  ``xp`` and
    ``fp`` are 1-D host arrays of equal length >= 1, copied into the node.  Unlike numpy, which returns garbage there, an
    ``xp`` that is not non-decreasing or holds a NaN or an infinity raises ValueError; ``period=`` is not supported."""
    if period is not None:
        raise TypeError("np.interp: period= is not supported on column expressions")
    if isinstance(xp, ColumnExpr) or isinstance(fp, ColumnExpr):
        raise TypeError("np.interp: xp and fp must be host arrays, only x can be a column expression")
    if not isinstance(x, ColumnExpr):
        raise TypeError("np.interp: x must be a column expression here (a host array cannot be mixed in)")
    xp, fp = np.asarray(xp, dtype=np.float64), np.asarray(fp, dtype=np.float64)
    if xp.ndim != 1 or fp.ndim != 1 or xp.size != fp.size or xp.size < 1:
        raise ValueError("np.interp: xp and fp must be 1-D arrays of equal length >= 1")
    if not np.all(np.isfinite(xp)) or np.any(xp[1:] < xp[:-1]):
        raise ValueError("np.interp: xp must be finite and non-decreasing")
    return lookup("INTERP", Table("INTERP", (xp, fp), xp.size, left=fp[0] if left is None else left,
                                  right=fp[-1] if right is None else right), x)


def _clip(a, a_min=None, a_max=None, **kwargs):
    """np.clip as numpy defines it, minimum(maximum(a, a_min), a_max): NaN in ``a`` or in a bound comes out, and the
    zeros keep numpy's signs, which a chain of where() would not."""
    if "min" in kwargs or "max" in kwargs:
        a_min, a_max = kwargs.pop("min", a_min), kwargs.pop("max", a_max)
    if kwargs:
        raise TypeError("np.clip: %s= is not supported on column expressions" % ", ".join(sorted(kwargs)))
    if a_min is None and a_max is None:
        raise ValueError("One of max or min must be given")
    out = _wrap(a)
    if a_min is not None:
        out = ColumnExpr._binary("MAX", out, a_min)
    if a_max is not None:
        out = ColumnExpr._binary("MIN", out, a_max)
    return out
