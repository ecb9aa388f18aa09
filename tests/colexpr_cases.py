"""Inputs and expressions shared by tests/test_colexpr_cpu.py (the g++ build of csrc/colexpr.hpp) and tests/test_gpu_colexpr.py
(the kernel): every entry of EXACT is a function of an attribute bag ``p`` with a, b, c, d that works on host vectors
(numpy gives the expected values) and on column-expression leaves alike."""

import numpy as np

SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072009e-308, -1e-310,
                     np.finfo(float).max, -np.finfo(float).max, 1.0, -1.0, 0.5, 2.0, 0.3])
NAMES = ["a", "b", "c", "d"]


def special_rows():
    """(256, 4): every pair of SPECIALS in (a, b); c and d walk through them too"""
    k = len(SPECIALS)
    S = np.empty((k * k, 4))
    S[:, 0] = np.repeat(SPECIALS, k)
    S[:, 1] = np.tile(SPECIALS, k)
    S[:, 2] = np.roll(np.tile(SPECIALS, k), 5)
    S[:, 3] = np.roll(np.repeat(SPECIALS, k), 3)
    return S


def inputs(n_random=4099, seed=20240611):
    """(X, weights, loglikes): n_random random rows (columns of different scales, every 7th row with a == b an integer:
    exact ties for == and <=) followed by special_rows()"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_random, 4)) * np.array([1.0, 3.0, 1e3, 1e-3])
    X[::7, 1] = np.round(X[::7, 1])
    X[::7, 0] = X[::7, 1]
    X = np.vstack([X, special_rows()])
    w = rng.integers(1, 5, len(X)).astype(float)
    ll = rng.standard_normal(len(X)) ** 2
    return X, w, ll


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


EXACT = {
    "add": lambda p: p.a + p.b, "sub": lambda p: p.a - p.b, "mul": lambda p: p.a * p.b, "div": lambda p: p.a / p.b,
    "radd": lambda p: 0.1 + p.a, "rsub": lambda p: 1.0 - p.c, "rmul": lambda p: 3.0 * p.d, "rdiv": lambda p: 1.0 / p.a,
    "sqrt": lambda p: np.sqrt(p.b), "square": lambda p: np.square(p.c), "reciprocal": lambda p: np.reciprocal(p.a),
    "negative": lambda p: -p.a, "absolute": lambda p: abs(p.a), "positive": lambda p: +p.a,
    "minimum": lambda p: np.minimum(p.a, p.b), "maximum": lambda p: np.maximum(p.a, p.b),
    "minimum_const": lambda p: np.minimum(p.a, 0.0), "maximum_const": lambda p: np.maximum(-0.0, p.a),
    "clip": lambda p: np.clip(p.a, -0.5, 0.5),
    "lt": lambda p: p.a < p.b, "le": lambda p: p.a <= p.b, "gt": lambda p: p.a > p.b, "ge": lambda p: p.a >= p.b,
    "eq": lambda p: p.a == p.b, "ne": lambda p: p.a != p.b,
    "and": lambda p: (p.a > 0) & (p.b < 1), "or": lambda p: (p.a > 0) | (p.b < 1), "not": lambda p: ~(p.a > p.c),
    "logical_and": lambda p: np.logical_and(p.a, p.b), "logical_or": lambda p: np.logical_or(p.a, p.b),
    "logical_not": lambda p: np.logical_not(p.a),
    "where": lambda p: np.where(p.a > p.b, p.c, p.d), "where_float_cond": lambda p: np.where(p.a, p.b, -p.b),
    "pow2": lambda p: p.a ** 2, "pow_half": lambda p: p.b ** 0.5, "pow_m1": lambda p: p.a ** -1, "pow1": lambda p: p.a ** 1,
    "bool_arith": lambda p: (p.a > 0) * p.b + (p.c < 0),
    "s8": lambda p: p.a * np.sqrt(abs(p.b) / 0.3) - p.c,
    "nested": lambda p: np.where((p.a > 0.1) & ~(p.b < -1), np.maximum(p.c, p.d) / (1.0 + p.a * p.a), -abs(p.d - p.c) * 0.5),
}
# programs of ONE op (plus its leaves): the ones that also run at the small row counts
ONE_OP = ["add", "sub", "mul", "div", "sqrt", "square", "reciprocal", "negative", "absolute", "minimum", "maximum", "lt", "le",
          "gt", "ge", "eq", "ne", "logical_and", "logical_or", "logical_not", "where_float_cond"]


def depth16(p):
    """a right-nested chain of 16 leaves: the stack gets 16 deep (products and differences: the order shows)"""
    xs = [p.a, p.b, p.c, p.d] * 4
    out = xs[-1]
    for k, x in enumerate(reversed(xs[:-1])):
        out = x - out if k % 2 else x * out
    return out


def code128(p):
    """128 instructions: 64 leaves, 63 binary ops, one negation"""
    xs = [p.a, p.b, p.c, p.d, 0.5, p.b, 1.5, p.a] * 8
    out = xs[0]
    for k, x in enumerate(xs[1:]):
        out = (out + x, out * x, out - x, np.maximum(out, x))[k % 4]
    return -out


COMPOSITES = {"depth16": depth16, "code128": code128}
