"""Shared by the CPU and GPU tests of the device-side edits of a sample set (gd_select_samples, gd_set_weights and the
mutators of chains.py routed through them): the inputs, every mutator as (the call on an MCSamples, the same edit made with
numpy on the inputs), and ``FakeSelectContext``, the numpy stand-in of the CPU tier with ``select_samples`` and
``set_weights``."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from fake_ctx import FakeContext  # noqa: E402
from test_devinput_cpu import FakeDevContext  # noqa: E402

from getdist_amd import _lib  # noqa: E402

NAMES = ["x", "y", "z", "k"]
CHAIN_ROWS = (700, 701, 650)
SETTINGS = dict(min_weight_ratio=-1)  # (zero weights stay until deleteZeros removes them)


def inputs(kind):
    """dict(samples, weights, loglikes): ``single`` one (1500, 4) array, ``chains`` three chains.  Integer weights 0..4 (so
    that thinning applies and deleteZeros has rows to delete), loglikes, and a column k of zeros and ones (the rows with
    k == 1 make it a fixed parameter)."""
    r = np.random.default_rng(20261020)
    out = []
    for k, rows in enumerate((1500,) if kind == "single" else CHAIN_ROWS):
        g = r.standard_normal((rows, 3))
        s = g @ np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.5, 0.9]]).T + [0.0, 1.0 + 0.05 * k, -2.0]
        s = np.column_stack([s, (r.random(rows) < 0.6).astype(float)])
        out.append((s, r.integers(0, 5, rows).astype(float), 0.5 * np.sum(g**2, axis=1)))
    if kind == "single":
        return dict(samples=out[0][0], weights=out[0][1], loglikes=out[0][2])
    return dict(samples=[c[0] for c in out], weights=[c[1] for c in out], loglikes=[c[2] for c in out])


def stacked(inp):
    """(S, w, ll, chain offsets or None) of the inputs as the object holds them"""
    if isinstance(inp["samples"], list):
        offs = np.cumsum([0] + [len(c) for c in inp["samples"]])
        return np.vstack(inp["samples"]), np.concatenate(inp["weights"]), np.concatenate(inp["loglikes"]), offs
    return inp["samples"], inp["weights"], inp["loglikes"], None


def split(S, w, ll, offs):
    """the constructor's arguments for the edited arrays: per-chain lists where there are chains"""
    if offs is None:
        return dict(samples=S, weights=w, loglikes=ll)
    cut = [slice(a, b) for a, b in zip(offs[:-1], offs[1:])]
    return dict(samples=[S[c] for c in cut], weights=None if w is None else [w[c] for c in cut], loglikes=[ll[c] for c in cut])


def thin_indices(factor, w):
    from oracle import convergence_oracle as co

    return np.asarray(co.thin_indices(factor, w), dtype=np.int64)


def _rows(S, w, ll, offs, ix, new_offs):
    return S[ix], w[ix], ll[ix], new_offs, NAMES


def _by_mask(S, w, ll, offs, mask):
    new = None if offs is None else np.cumsum([0] + [int(np.count_nonzero(mask[a:b])) for a, b in zip(offs[:-1], offs[1:])])
    return _rows(S, w, ll, offs, mask, new)


def _burn(frac):
    def expect(S, w, ll, offs):
        ix = int(round(len(S) * frac))
        return _rows(S, w, ll, offs, slice(ix, None), None if offs is None else np.unique(np.maximum(offs - ix, 0)))

    return expect


def _thin(S, w, ll, offs):
    ix = thin_indices(2, w)
    return S[ix], None, ll[ix], None if offs is None else np.searchsorted(ix, offs), NAMES


def _weighted_thin(S, w, ll, offs):
    rows, counts, lens = [], [], [0]
    for a, b in ([(0, len(S))] if offs is None else zip(offs[:-1], offs[1:])):
        u, c = np.unique(thin_indices(2, w[a:b]) + a, return_counts=True)
        rows.append(u), counts.append(c), lens.append(len(u))
    rows = np.concatenate(rows)
    return S[rows], np.concatenate(counts).astype(float), ll[rows], None if offs is None else np.cumsum(lens), NAMES


def _fixed(S, w, ll, offs):
    S, w, ll, offs, _ = _by_mask(S, w, ll, offs, S[:, 3] == 1.0)
    return S, w, ll, offs, NAMES  # (the constructor of the yardstick object takes the constant column out itself)


def _apply_fixed(mc):
    mc.filter(mc.getDeviceParams().k == 1.0)
    assert mc.deleteFixedParams() == ([3], [1.0])


EXTRA_LOGLIKES = lambda n: 0.25 * np.cos(np.arange(n) * 0.37) + 0.3  # noqa: E731


def _reweight(S, w, ll, offs):
    extra = EXTRA_LOGLIKES(len(S))
    return S, w * np.exp(-(extra - np.min(extra))), ll + extra, offs, NAMES


def _cool(S, w, ll, offs):
    new = ll * 2.0
    return S, w * np.exp(-(new - ll) - (np.min(ll) * (1 - 2.0))), new, offs, NAMES


def _expr(mc):
    p = mc.getDeviceParams()
    return p.x * p.y + 1.0


# name -> (the call, the same edit on (S, w, ll, chain offsets) -> (S, w, ll, offsets, names), the rows or columns change)
MUTATORS = {
    "filter_mask": (lambda mc: mc.filter(stacked_of(mc)[:, 0] > 0.1), lambda S, w, ll, o: _by_mask(S, w, ll, o, S[:, 0] > 0.1), True),
    "filter_index": (lambda mc: mc.filter(np.arange(0, mc.numrows, 3)),
                     lambda S, w, ll, o: _rows(S, w, ll, o, np.arange(0, len(S), 3),
                                               None if o is None else np.searchsorted(np.arange(0, len(S), 3), o)), True),
    "filter_expr": (lambda mc: mc.filter(mc.getDeviceParams().y > 1.25), lambda S, w, ll, o: _by_mask(S, w, ll, o, S[:, 1] > 1.25), True),
    "deleteZeros": (lambda mc: mc.deleteZeros(), lambda S, w, ll, o: _by_mask(S, w, ll, o, w > 0), True),
    "setMinWeightRatio": (lambda mc: mc.setMinWeightRatio(0.3), lambda S, w, ll, o: _by_mask(S, w, ll, o, w > 0.3 * np.max(w)), True),
    "removeBurn": (lambda mc: mc.removeBurn(0.3), _burn(0.3), True),
    "removeBurnFraction": (lambda mc: mc.removeBurnFraction(0.2), _burn(0.2), True),
    "thin": (lambda mc: mc.thin(2), _thin, True),
    "weighted_thin": (lambda mc: mc.weighted_thin(2), _weighted_thin, True),
    "deleteFixedParams": (_apply_fixed, _fixed, True),
    "addDerived_vector": (lambda mc: mc.addDerived(np.sin(np.arange(mc.numrows) * 0.1), "s"),
                          lambda S, w, ll, o: (np.column_stack([S, np.sin(np.arange(len(S)) * 0.1)]), w, ll, o, NAMES + ["s"]), True),
    "addDerived_expr": (lambda mc: mc.addDerived(_expr(mc), "xy1"),
                        lambda S, w, ll, o: (np.column_stack([S, S[:, 0] * S[:, 1] + 1.0]), w, ll, o, NAMES + ["xy1"]), True),
    "reweightAddingLogLikes": (lambda mc: mc.reweightAddingLogLikes(EXTRA_LOGLIKES(mc.numrows)), _reweight, False),
    "cool": (lambda mc: mc.cool(2.0), _cool, False),
}


def stacked_of(mc):
    """the object's sample values WITHOUT touching its host mirror: the inputs it was built from, kept by the test"""
    return mc._test_inputs


def make(cls, inp, wrap=None, **kw):
    """the inputs as an MCSamples (``wrap``: what turns an array into a device buffer; None: host arrays)"""
    w = (lambda v: [w(a) for a in v] if isinstance(v, list) else wrap(v)) if wrap else (lambda v: v)
    mc = cls(samples=w(inp["samples"]), weights=w(inp["weights"]), loglikes=w(inp["loglikes"]), names=list(NAMES),
             settings=dict(SETTINGS), **kw)
    mc._test_inputs = stacked(inp)[0]
    return mc


def expected(cls, name, inp, **kw):
    """the yardstick: a fresh MCSamples of the numpy-edited inputs"""
    S, w, ll, offs, names = MUTATORS[name][1](*stacked(inp))
    return cls(names=list(names), settings=dict(SETTINGS), **split(np.ascontiguousarray(S), w, ll, offs), **kw)


# ---- the CPU tier's context double -----------------------------------------------------------------------------------------
class ExprOps:
    """the few ops of Context.expr_eval the cases use, on a double's host columns"""

    def expr_eval(self, code, consts, dst, dst_arg=0, lo=0, hi=None, stats=False, tables=None):
        assert not stats and not tables and (lo, hi) in ((0, None), (0, self.N))
        binary = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "GT": np.greater, "LT": np.less, "EQ": np.equal}
        stack = []
        for op, arg in np.asarray(code).reshape(-1, 2):
            name = _lib.GD_EX_OPS[op]
            if name == "COL":
                stack.append(self.s[:, arg].copy())
            elif name == "CONST":
                stack.append(np.full(self.N, consts[arg]))
            else:
                b, a = stack.pop(), stack.pop()
                stack.append(binary[name](a, b).astype(np.float64))
        (out,) = stack
        if dst == _lib.GD_EX_TO_COLUMN:
            self.s[:, self.n + dst_arg] = out
            return self.n + dst_arg
        assert dst in (_lib.GD_EX_TO_HOST_F64, _lib.GD_EX_TO_HOST_U8)
        return out if dst == _lib.GD_EX_TO_HOST_F64 else (out != 0).astype(np.uint8)


class FakeHostContext(ExprOps, FakeContext):
    """the host route's double: no ``select_samples``, no ``set_weights``"""


class FakeSelectContext(ExprOps, FakeDevContext):
    """FakeDevContext with the two edits of the resident set, made with numpy"""

    selects = weight_sets = 0

    def _refuse(self, msg):
        raise _lib.GdhipError(_lib.GD_ERR_BADARG, msg)

    def select_samples(self, rows=None, keep_cols=None, append=None, weights="keep"):
        N = self.N
        kind = "all" if rows is None else rows[0]
        if kind == "all":
            ix = np.arange(N)
        elif kind == "range":
            if not 0 <= rows[1] < rows[2] <= N:
                self._refuse("gd_select_samples: row range")
            ix = np.arange(rows[1], rows[2])
        elif kind == "mask":
            m = np.asarray(rows[1].a if hasattr(rows[1], "a") else rows[1])
            assert m.shape == (N,)
            ix = np.flatnonzero(m != 0)
        elif kind == "weight_gt":
            ix = np.flatnonzero((np.ones(N) if self.w is None else self.w) > rows[1])
        else:
            assert kind == "rows"
            ix = np.asarray(rows[1].a[:rows[2]] if hasattr(rows[1], "a") else rows[1], dtype=np.int64)
            if ix.size and (ix.min() < 0 or ix.max() >= N):
                self._refuse("gd_select_samples: row outside the set")
        if ix.size == 0:
            self._refuse("gd_select_samples: no rows selected")
        cols = list(range(self.n)) if keep_cols is None else [int(c) for c in keep_cols]
        assert cols == sorted(set(cols)) and all(0 <= c < self.n for c in cols)
        parts = [self.s[ix][:, cols]]
        if isinstance(append, tuple):
            parts.append(self.s[ix, self.n + append[1]].reshape(-1, 1))
        elif append is not None:
            assert np.shape(append) == (N,)
            parts.append(np.asarray(append, dtype=np.float64)[ix].reshape(-1, 1))
        if isinstance(weights, str):
            w = self.w[ix] if (weights == "keep" and self.w is not None) else None
        else:
            w = np.array(weights, dtype=np.float64)
            assert w.shape == (ix.size,)
        FakeContext.upload(self, np.hstack(parts), w)
        type(self).selects += 1
        return self.N

    def set_weights(self, w):
        assert not getattr(self, "_w_sel", 0)
        self.w = None if w is None else np.array(w, dtype=np.float64)
        assert self.w is None or self.w.shape == (self.N,)
        self.weighted = self.w is not None
        self._like_w = None
        type(self).weight_sets += 1

    def read_column(self, j):
        return self.s[:, j].copy()
