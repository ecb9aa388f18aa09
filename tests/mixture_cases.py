"""Cases, truths and the numpy context double of the gaussian_mixtures tests.

- ``specs()``: the mixtures of tests/golden/mixtures.npz as constructor arguments (written to tests/golden/mixtures.json by
  tests/golden/make_golden_mixtures.py; the tests build from the JSON, so file and recorded numbers travel together);
- ``MixtureFakeContext``: tests/fake_ctx.FakeContext plus ``mixture_nll``, the whitened max-shifted log-sum-exp in numpy;
- ``truth_nll`` / ``reference_formula_nll``: the extended-precision truth of the GPU tests and the reference's own float64
  formula, whose error against that truth sets the tolerance;
- ``kde_truth_cases`` / ``kde_stats``: the KDE-against-the-drawn-distribution cases and their statistics."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_NPZ = os.path.join(HERE, "golden", "mixtures.npz")
GOLDEN_JSON = os.path.join(HERE, "golden", "mixtures.json")
KDE_JSON = os.path.join(HERE, "golden", "mixtures_kde_oracle.json")


def specs():
    """name -> dict(cls, args, sim, and what to record)"""
    r = np.random.default_rng(np.random.SeedSequence([20261016, 31]))
    d = 12
    covs12 = []
    for scale in (1.0, 0.5):
        A = r.normal(size=(d, d)) * 0.3 + np.diag(np.linspace(0.8, 1.6, d))
        covs12.append((scale * A @ A.T).tolist())
    means12 = [r.normal(size=d).tolist(), (r.normal(size=d) + 1.5).tolist()]
    return {
        "mix1d": dict(cls="Mixture1D", args=dict(means=[0.0, 2.5], sigmas=[1.0, 0.6], weights=[0.7, 0.3], xmin=-1.0),
                      sim=dict(size=1500, seed=11), marged=[0], density1d=[0], density2d=[], marg=[], cond=[]),
        "mix2d": dict(cls="Mixture2D",
                      args=dict(means=[[0.0, 0.0], [2.0, 1.0], [-1.5, 2.0]],
                                covs=[[1.0, 0.5, 0.3], [[0.5, 0.1], [0.1, 0.8]], [0.4, 0.9, -0.6]],
                                weights=[0.5, 0.3, 0.2], ymax=3.0),
                      sim=dict(size=2000, seed=12), marged=[1], density1d=[1], density2d=[None], marg=[[1]], cond=[]),
        "rand4": dict(cls="RandomTestMixtureND", args=dict(ndim=4, ncomponent=3, seed=5),
                      sim=dict(size=2000, seed=13), marged=[2], density1d=[1], density2d=[[0, 2]],
                      marg=[[0, 2], [1], [3, 0, 1]], cond=[[[1, 3], [0.4, 0.6]], [[0], [0.2]]]),
        "g12": dict(cls="MixtureND", args=dict(means=means12, covs=covs12, weights=[2.0, 1.0],
                                                names=["q%d" % i for i in range(d)]),
                    sim=dict(size=1000, seed=14), marged=[7], density1d=[3], density2d=[[2, 9]],
                    marg=[[2, 9], [0, 4, 11]], cond=[[[0, 1, 2, 3, 4, 5], [0.1, -0.2, 0.3, 0.0, 0.5, -0.4]]]),
    }


def load_specs():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


def build(module, spec):
    """The mixture of a spec from ``module`` (this package's gaussian_mixtures, or the reference's)."""
    return getattr(module, spec["cls"])(**spec["args"])


MARGED_X = np.linspace(-2.5, 4.0, 53)


def record(mix, spec):
    """Everything the golden file holds for one mixture (run on the reference when regenerating, on this package when
    comparing): name -> array."""
    out = {}
    rows = mix.sim(spec["sim"]["size"], spec["sim"]["seed"])
    out["sim"] = rows
    out["pdf"] = mix.pdf(rows if mix.dim > 1 else rows[:, 0])
    out["autoRanges"] = np.array(mix.autoRanges(), dtype=np.float64)
    for i in spec["marged"]:
        out["pdf_marged/%d" % i] = mix.pdf_marged(i, MARGED_X)
    for i in spec["density1d"]:
        dens = mix.density1D(i)
        out["density1D/%d/x" % i], out["density1D/%d/P" % i] = np.array(dens.x), np.array(dens.P)
    for n, params in enumerate(spec["density2d"]):
        dens = mix.density2D(params, num_points=64)
        out["density2D/%d/x" % n], out["density2D/%d/y" % n] = np.array(dens.x), np.array(dens.y)
        out["density2D/%d/P" % n] = np.array(dens.P)
    for n, params in enumerate(spec["marg"]):
        m = mix.marginalizedMixture(params)
        out["marg/%d/means" % n], out["marg/%d/covs" % n] = np.array(m.means), np.array(m.covs)
        out["marg/%d/weights" % n] = np.array(m.weights)
    for n, (fixed, values) in enumerate(spec["cond"]):
        m = mix.conditionalMixture(fixed, values)
        out["cond/%d/means" % n], out["cond/%d/covs" % n] = np.array(m.means), np.array(m.covs)
        out["cond/%d/weights" % n] = np.array(m.weights)
    return out


# ---- the whitened log-sum-exp in numpy (the context double) and in extended precision (the truth) -------------------
def whitened_nll(x, means, whiten, logcoef, dtype=np.float64):
    """-log sum_k exp(logcoef_k - 1/2 |W_k (x - mu_k)|^2) per row of x (rows x d), max-shifted"""
    x = np.asarray(x, dtype=dtype)
    t = np.empty((len(logcoef), x.shape[0]), dtype=dtype)
    for k in range(len(logcoef)):
        y = (x - np.asarray(means[k], dtype=dtype)) @ np.asarray(whiten[k], dtype=dtype).T
        t[k] = dtype(logcoef[k]) - np.sum(y * y, axis=1) / 2
    m = np.max(t, axis=0)
    return -(m + np.log(np.sum(np.exp(t - m), axis=0)))


def _fake_base():
    sys.path.insert(0, HERE)
    from fake_ctx import FakeContext

    return FakeContext


def fake_context_class():
    """FakeContext + mixture_nll (made on demand: importing fake_ctx pulls in the oracle and scipy)."""

    class MixtureFakeContext(_fake_base()):
        mixture_calls = 0

        def mixture_nll(self, cols, means, whiten, logcoef, lo=0, hi=None):
            type(self).mixture_calls += 1
            hi = self.N if hi is None else hi
            cols = np.asarray(cols, dtype=int)
            means, whiten, logcoef = np.asarray(means, float), np.asarray(whiten, float), np.asarray(logcoef, float)
            if not (0 <= lo < hi <= self.N) or cols.size < 1 or np.any(cols < 0) or np.any(cols >= self.n):
                raise RuntimeError("libgdhip error -1: bad argument")
            assert means.shape == (logcoef.size, cols.size) and whiten.shape == (logcoef.size, cols.size, cols.size)
            return whitened_nll(self.s[lo:hi][:, cols], means, np.tril(whiten), logcoef)

    return MixtureFakeContext


def _ld_cholesky(a):
    """Cholesky factor of a symmetric positive definite matrix in np.longdouble (numpy's LAPACK path is float64 only)"""
    a = np.asarray(a, dtype=np.longdouble)
    n = a.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        s = a[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (a[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def truth_nll(x, means, covs, weights):
    """Extended-precision truth: per component a longdouble Cholesky factor, chi^2 by forward substitution, log norm from
    the factor's diagonal, then a max-shifted log-sum-exp; float64 result of the longdouble value."""
    ld = np.longdouble
    x = np.asarray(x, dtype=ld)
    N, d = x.shape
    w = np.asarray(weights, dtype=ld)
    w = w / np.sum(w)
    t = np.empty((len(w), N), dtype=ld)
    for k in range(len(w)):
        L = _ld_cholesky(covs[k])
        dx = (x - np.asarray(means[k], dtype=ld)).T  # d x N
        y = np.zeros((d, N), dtype=ld)
        for i in range(d):  # forward substitution L y = dx
            y[i] = (dx[i] - L[i, :i] @ y[:i]) / L[i, i]
        lognorm = ld(d) / 2 * np.log(2 * ld(np.pi)) + np.sum(np.log(np.diag(L)))
        t[k] = np.log(w[k]) - lognorm - np.sum(y * y, axis=0) / 2
    m = np.max(t, axis=0)
    return -(m + np.log(np.sum(np.exp(t - m), axis=0)))


def reference_formula_nll(x, mix):
    """-log(pdf) as the reference forms it (float64, inverse covariances, one einsum per component); inf where it
    underflows"""
    with np.errstate(divide="ignore"):
        flat = type(mix).__name__ in ("Mixture1D", "Gaussian1D")  # (their pdf takes the values, not rows of one column)
        return -np.log(mix.pdf(np.asarray(x)[:, 0] if flat else np.asarray(x)))


# ---- KDE against the distribution the samples were drawn from ------------------------------------------------------------
KDE_ROWS = 1_000_000


def kde_truth_cases(module):
    """name -> (mixture, seed)"""
    return {
        "gaussian2d": (module.Gaussian2D([0.3, -0.2], [1.0, 0.7, 0.6]), 101),
        "bimodal_ymax": (module.Mixture2D([[-1.0, 0.0], [1.5, 0.8]], [[0.6, 0.5, 0.4], [0.5, 0.7, -0.5]], weights=[0.6, 0.4],
                                          ymax=1.6), 102),
    }


def kde_stats(x, y, P, mix):
    """(max |P - truth| / max truth, integrated |P - truth|) with both normalised to unit trapezoid integral on the grid"""
    from getdist_amd.densities import Density2D

    xx, yy = np.meshgrid(x, y)
    truth = Density2D(x, y, mix.pdf(xx, yy))
    truth.normalize("integral", in_place=True)
    est = Density2D(x, y, np.array(P, dtype=np.float64))
    est.normalize("integral", in_place=True)
    diff = np.abs(est.P - truth.P)
    return float(np.max(diff) / np.max(truth.P)), float(truth.integrate(diff))
