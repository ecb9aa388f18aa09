"""GPU tier of getdist_amd.gaussian_mixtures: gd_mixture_nll against an extended-precision host truth, bit-equal reruns,
MCSamples(logLikes=True) and prior re-weighting end to end, and the 2D KDE against the distribution the rows were drawn
from (the yardstick that does not go through the oracle's restatement of the KDE).

Tolerance of the device log-pdf (not fitted to the device): the reference's own formula, -log(pdf) in float64 with explicit
inverse covariances, is evaluated on the same inputs and its error against the truth measured where it is finite; the
device, which uses a different but equally valid factorisation (whitening by the inverse Cholesky factor), may err by at
most 4 x that -- a factor, because both errors scale with the condition number --, with a floor of 8 ulp of the largest
result (the d = 1 cases, where the reference formula is nearly exact).  Every case prints reference error, device error
and their ratio (run with -s; profiles/mixture_gpu_tests.txt keeps one such run)."""

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mixture_cases as mcases  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
N_ROWS = 20_011  # not a multiple of 64, 128 or 256 (the rows of a block)
N_COLS = 200


@pytest.fixture(scope="module")
def resident():
    """One context holding N_ROWS x 200 correlated columns, and the host copy."""
    from getdist_amd._lib import Context

    r = np.random.default_rng(np.random.SeedSequence([20261016, 41]))
    s = r.standard_normal((N_ROWS, N_COLS)) * r.uniform(0.5, 2.0, N_COLS) + r.normal(size=N_COLS)
    s[:, 1:] += 0.5 * s[:, :-1]
    s = np.asfortranarray(s)
    ctx = Context(0)
    ctx.upload(s)
    yield ctx, s
    ctx.close()


def _mixture(s, d, K, seed):
    """K components in d dimensions over a scattered choice of the resident columns; means within a sigma of the columns'
    means and covariances D A A^T D (D: the columns' standard deviations, A = 1 + 0.3 G / sqrt(d), condition number of a
    few) times 1..3, so every row is a few sigma from some component and the reference formula stays finite"""
    from getdist_amd import gaussian_mixtures as gm

    r = np.random.default_rng(np.random.SeedSequence([20261016, 42, d, K, seed]))
    cols = np.sort(r.choice(N_COLS, size=d, replace=False))[::-1].copy() if d < N_COLS else r.permutation(N_COLS)
    mu, sd = s[:, cols].mean(axis=0), s[:, cols].std(axis=0)
    means, covs = [], []
    for k in range(K):
        A = 0.3 * r.normal(size=(d, d)) / np.sqrt(d) + np.eye(d)
        covs.append(A @ A.T * np.outer(sd, sd) * r.uniform(1.0, 3.0))
        means.append(mu + r.normal(size=d) * 0.5 * sd)
    weights = r.uniform(0.5, 1.5, K)
    return gm.MixtureND(means, covs, weights), cols


def _check(ctx, s, mix, cols, lo=0, hi=None, label="", require_finite_reference=True):
    hi = N_ROWS if hi is None else hi
    x = s[lo:hi][:, cols]
    whiten, logcoef = mix._whitened()
    got = np.array(ctx.mixture_nll(cols, mix.means, whiten, logcoef, lo=lo, hi=hi))
    assert got.shape == (hi - lo,) and np.all(np.isfinite(got))
    truth = mcases.truth_nll(x, mix.means, mix.covs, mix.weights)
    ref = mcases.reference_formula_nll(x, mix)
    ok = np.isfinite(ref)
    assert ok.all() or not require_finite_reference
    ref_err = float(np.max(np.abs(ref[ok] - truth[ok]))) if ok.any() else float("nan")
    dev_err = float(np.max(np.abs(got.astype(np.longdouble) - truth)))
    floor = 8 * EPS * float(np.max(np.abs(truth)))
    print("mixture_nll %-28s rows %6d  reference error %.3e  device error %.3e  ratio %.3f  floor %.3e"
          % (label, hi - lo, ref_err, dev_err, dev_err / ref_err if ref_err > 0 else float("inf"), floor))
    return got, truth, ref_err, dev_err, floor


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("d", [1, 2, 3, 17, 50, 64, 65, 200])
def test_mixture_nll_against_extended_precision_truth(resident, d, K):
    ctx, s = resident
    mix, cols = _mixture(s, d, K, 0)
    hi = 6_007 if d == 200 else None  # (the longdouble truth of 200 columns is slow on the host)
    _, _, ref_err, dev_err, floor = _check(ctx, s, mix, cols, hi=hi, label="d=%d K=%d" % (d, K))
    assert dev_err <= max(4 * ref_err, floor)


def test_sub_range_of_rows(resident):
    ctx, s = resident
    mix, cols = _mixture(s, 17, 3, 1)
    part, _, ref_err, dev_err, floor = _check(ctx, s, mix, cols, lo=777, hi=12_345, label="d=17 K=3 rows 777..12345")
    assert dev_err <= max(4 * ref_err, floor)
    whiten, logcoef = mix._whitened()
    whole = np.array(ctx.mixture_nll(cols, mix.means, whiten, logcoef))
    assert np.array_equal(whole[777:12_345], part)  # a row's value does not depend on where its block starts
    one = np.array(ctx.mixture_nll(cols, mix.means, whiten, logcoef, lo=N_ROWS - 1, hi=N_ROWS))
    assert np.array_equal(one, whole[-1:])


def test_ill_conditioned_covariance():
    """In-block correlation 0.995 (synth.RHO_CYCLE): the condition number of a 5-block is ~1000 and both errors grow by it.
    The rows are drawn from the mixture itself (a context of this test's own), so that they lie along its narrow directions
    and the reference formula is finite on all of them."""
    from getdist_amd import gaussian_mixtures as gm
    from getdist_amd import synth
    from getdist_amd._lib import Context

    rho = synth.RHO_CYCLE[5]
    assert rho == 0.995
    d = 10
    sig = np.linspace(0.5, 2.0, d)
    corr = np.eye(d)
    for b in range(0, d, 5):
        corr[b:b + 5, b:b + 5] = rho + (1 - rho) * np.eye(5)
    cov = corr * np.outer(sig, sig)
    assert np.linalg.cond(cov) > 1000
    mix = gm.MixtureND([np.zeros(d), np.ones(d) * 0.3], [cov, cov * 1.7], [0.4, 0.6])
    s = np.asfortranarray(mix.sim(N_ROWS, 23))
    ctx = Context(0)
    try:
        ctx.upload(s)
        _, _, ref_err, dev_err, floor = _check(ctx, s, mix, np.arange(d), label="rho=0.995 d=10 K=2")
    finally:
        ctx.close()
    assert dev_err <= max(4 * ref_err, floor)


def test_rows_40_sigma_out_stay_finite(resident):
    """Means 40 sigma from the rows: the reference's -log(pdf) is inf (exp underflows beyond chi^2 ~ 1490); the device
    value must be finite and match the truth.  With no finite reference error to scale, the bound is the a-priori one of
    the whitened sum: each of the d y_i carries at most (i + 2) roundings of relative size eps amplified by the condition
    number kappa of the factor, so |error| <= 4 (d + 2) eps kappa |truth| (4: the squares and their sum, with margin)."""
    from getdist_amd import gaussian_mixtures as gm

    ctx, s = resident
    cols = np.array([3, 50, 120])
    sd = s[:, cols].std(axis=0)
    corr = np.array([[1.0, 0.3, -0.2], [0.3, 1.0, 0.4], [-0.2, 0.4, 1.0]])
    cov = corr * np.outer(sd, sd)
    kappa = np.linalg.cond(np.linalg.cholesky(cov))
    far = s[:, cols].mean(axis=0) + 40 * sd
    for K, mix in ((1, gm.GaussianND(far, cov)), (2, gm.MixtureND([far, far + sd], [cov, 1.2 * cov], [0.5, 0.5]))):
        got, truth, _, dev_err, _ = _check(ctx, s, mix, cols, label="40 sigma out K=%d" % K, require_finite_reference=False)
        assert np.all(np.isinf(mcases.reference_formula_nll(s[:, cols], mix)))
        assert np.all(got > 1490 / 2)
        assert dev_err <= 4 * (3 + 2) * EPS * kappa * float(np.max(np.abs(truth)))


def test_two_runs_bit_equal(resident):
    ctx, s = resident
    for d, K in ((3, 3), (50, 3), (200, 1)):
        mix, cols = _mixture(s, d, K, 2)
        whiten, logcoef = mix._whitened()
        a = np.array(ctx.mixture_nll(cols, mix.means, whiten, logcoef))
        b = np.array(ctx.mixture_nll(cols, mix.means, whiten, logcoef))
        assert np.array_equal(a, b)


def test_bad_arguments_return_status(resident):
    from getdist_amd._lib import GdhipError

    ctx, _ = resident
    one = (np.zeros((1, 2)), np.eye(2)[None], np.zeros(1))
    for cols, lo, hi in (([0, N_COLS], 0, None), ([0, -1], 0, None), ([0, 1], 5, 5), ([0, 1], 0, N_ROWS + 1), ([0, 1], -1, 4)):
        with pytest.raises(GdhipError):
            ctx.mixture_nll(cols, *one, lo=lo, hi=hi)
    with pytest.raises(ValueError):
        ctx.mixture_nll([0, 1], np.zeros((1, 3)), np.eye(2)[None], np.zeros(1))


def test_mcsamples_with_loglikes_on_device():
    mix = mcases.build(__import__("getdist_amd.gaussian_mixtures", fromlist=["x"]), mcases.load_specs()["rand4"])
    mc = mix.MCSamples(200_000, logLikes=True, random_state=7)
    rows = mix.sim(200_000, 7)
    assert np.array_equal(mc.samples, rows)
    want = -np.log(mix.pdf(rows))  # numpy, this package
    truth = mcases.truth_nll(rows, mix.means, mix.covs, mix.weights)
    ref_err = float(np.max(np.abs(want - truth)))
    dev_err = float(np.max(np.abs(mc.loglikes.astype(np.longdouble) - truth)))
    floor = 8 * EPS * float(np.max(np.abs(truth)))
    print("MCSamples(200000, logLikes=True): reference error %.3e  device error %.3e  max |device - numpy| %.3e"
          % (ref_err, dev_err, float(np.max(np.abs(mc.loglikes - want)))))
    assert dev_err <= max(4 * ref_err, floor)
    assert np.max(np.abs(mc.loglikes - want)) <= ref_err + max(4 * ref_err, floor)  # (triangle inequality through the truth)
    st = mc.getLikeStats()
    assert st is not None and np.isclose(st.logLike_sample, np.min(mc.loglikes), rtol=0, atol=0)


def test_prior_reweighting_end_to_end():
    """s ~ N(m0, C0) in 6 dimensions, re-weighted by a Gaussian prior N(mp, Cp) on columns (4, 0, 2).  The weighted
    distribution is the product of the two Gaussians: precision P0 + E^T Cp^-1 E (E picks the three columns), mean
    Sigma (P0 m0 + E^T Cp^-1 mp).  The weighted sample mean of column j has standard error sqrt(Sigma_jj / N_eff) with
    N_eff = (sum w)^2 / sum w^2 of the new weights (independent rows); 5 standard errors."""
    from getdist_amd import gaussian_mixtures as gm

    r = np.random.default_rng(17)
    A = r.normal(size=(6, 6)) * 0.4 + np.eye(6)
    C0, m0 = A @ A.T, r.normal(size=6)
    base = gm.GaussianND(m0, C0, names=["t%d" % i for i in range(6)])
    s = base.MCSamples(400_000, random_state=18)
    B = r.normal(size=(3, 3)) * 0.3 + np.eye(3)
    Cp, mp = B @ B.T * 0.8, m0[[4, 0, 2]] + np.array([0.4, -0.3, 0.5])
    prior = gm.GaussianND(mp, Cp, names=["t4", "t0", "t2"])
    s.reweightAddingLogLikes(prior.logLikes(s))
    E = np.zeros((3, 6))
    E[0, 4] = E[1, 0] = E[2, 2] = 1.0
    P0, Pp = np.linalg.inv(C0), np.linalg.inv(Cp)
    Sigma = np.linalg.inv(P0 + E.T @ Pp @ E)
    mean = Sigma @ (P0 @ m0 + E.T @ Pp @ mp)
    w = s.weights
    neff = np.sum(w) ** 2 / np.sum(w ** 2)
    pulls = (s.getMeans() - mean) / np.sqrt(np.diag(Sigma) / neff)
    print("prior re-weighting: N_eff %.0f of %d, pulls %s" % (neff, len(w), np.array2string(pulls, precision=2)))
    assert neff > 1000 and np.max(np.abs(pulls)) < 5
    assert np.max(np.abs(m0 - mean) / np.sqrt(np.diag(Sigma) / neff)) > 20  # (the prior did move the means)


def test_kde_against_the_distribution_drawn_from():
    """1e6 rows of a Gaussian2D and of a bimodal Mixture2D with ymax: get2DDensity, normalised by its integral, against the
    mixture's pdf on the same grid (normalised the same way).  The bound is the oracle's own distance from the truth on
    the same rows (tests/golden/mixtures_kde_oracle.json, made on the CPU by make_golden_mixtures.py) plus the project's
    grid parity of 1e-6."""
    from getdist_amd import gaussian_mixtures as gm

    with open(mcases.KDE_JSON) as f:
        recorded = json.load(f)
    for name, (mix, seed) in mcases.kde_truth_cases(gm).items():
        rec = recorded[name]
        assert rec["rows"] == mcases.KDE_ROWS and rec["seed"] == seed
        mc = mix.MCSamples(mcases.KDE_ROWS, random_state=seed)
        dens = mc.get2DDensity(mix.names[0], mix.names[1], normalized=True)
        assert (len(dens.x), len(dens.y)) == (rec["nx"], rec["ny"])
        rel_max, l1 = mcases.kde_stats(dens.x, dens.y, dens.P, mix)
        print("KDE vs truth %-13s device: max %.6e  L1 %.6e   oracle: max %.6e  L1 %.6e"
              % (name, rel_max, l1, rec["rel_max"], rec["l1"]))
        assert abs(rel_max - rec["rel_max"]) <= 1e-6 and abs(l1 - rec["l1"]) <= 1e-6
