"""GPU tier of MCSamples.copy (gd_clone_samples: the resident sample set duplicated device to device),
getCombinedSamplesWithSamples and the small queries around them, against the reference's outputs in
tests/golden/compose.npz and, parent against copy, against values taken before the copy was made.

Gates: means and covariance 1e-12 (tests/test_gpu_densities.py); scalars derived from the covariance or from N_eff 1e-9
(SURVEY.md 8d); density grids 1e-6 of their maximum; limits as test_marge_stats_golden gates them."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_cases as cc  # noqa: E402
import golden_util as gu  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_MOMENTS = 1e-12
TOL_SCALAR = 1e-9
TOL_GRID = 1e-6


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


def build(fx, **kw):
    from getdist_amd.mcsamples import MCSamples

    return cc.build(MCSamples, fx, **kw)


def device_rows(ctx, j):
    """Column j of the resident sample set (j = -2: the weights; None for a unit-weight set) read back from the device."""
    ptr = ctx.column_ptr(j)
    if not ptr:
        return None
    out = np.empty(ctx.N)
    ctx._check(ctx.lib.gd_memcpy_d2h(ctx.h, out.ctypes.data, ptr, out.nbytes))
    return out


def check_limits(par, want_rows, want_meanerr):
    got = cc.limit_rows(par)
    assert np.array_equal(got[:, 2:], want_rows[:, 2:]), "limit types"
    assert np.max(np.abs(got[:, :2] - want_rows[:, :2])) < 2e-5 * max(1e-300, float(par.err)), (got, want_rows)
    assert np.allclose([par.mean, par.err], want_meanerr, rtol=1e-11)


# ---- clone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", ["A", "U", "MC", "ONE"])
def test_clone_columns_and_weights(fx):
    s = build(fx)
    c = s.copy()
    assert c.ctx is not s.ctx and c.ctx.h != s.ctx.h
    assert (c.ctx.N, c.ctx.n, c.ctx.weighted) == (s.ctx.N, s.ctx.n, s.ctx.weighted) == (s.numrows, s.n, s.weights is not None)
    assert c.ctx.column_ptr(0) != s.ctx.column_ptr(0)
    for j in range(s.n):
        got = device_rows(c.ctx, j)
        assert np.array_equal(got, device_rows(s.ctx, j)) and np.array_equal(got, s.samples[:, j]), j
    if s.weights is None:
        assert device_rows(c.ctx, -2) is None and device_rows(s.ctx, -2) is None
    else:
        assert c.ctx.column_ptr(-2) != s.ctx.column_ptr(-2)
        assert np.array_equal(device_rows(c.ctx, -2), device_rows(s.ctx, -2))
        assert np.array_equal(device_rows(c.ctx, -2), s.weights)
    assert gu.relerr(c.ctx.cov()[1], s.fullcov) < TOL_MOMENTS
    assert c.ctx.weights_integral() == s.ctx.weights_integral()
    s.ctx.close(), c.ctx.close()


def test_clone_keeps_the_integral_weights_flag():
    s = build("B")
    c = s.copy()
    assert s.ctx.weights_integral() and c.ctx.weights_integral()
    assert c.ctx.weight_stats() == s.ctx.weight_stats()  # (integer weights: the sums are exact)
    real = build("A")
    assert not real.ctx.weights_integral() and not real.copy().ctx.weights_integral()


def test_clone_refuses_bad_arguments():
    from getdist_amd._lib import GD_ERR_BADARG, Context, GdhipError

    s = build("ONE")
    empty = Context(0)
    for dst, src in ((s.ctx, s.ctx), (s.ctx, empty)):
        with pytest.raises(GdhipError) as e:
            dst.clone_samples(src)
        assert e.value.code == GD_ERR_BADARG
    assert np.array_equal(device_rows(s.ctx, 0), s.samples[:, 0])  # a refused call leaves the destination as it was
    empty.close()


def test_copy_is_independent_of_the_parent():
    s = build("A")
    means, cov, dens = s.means.copy(), s.fullcov.copy(), s.get1DDensity("x").P.copy()
    c = s.copy()
    c.reweightAddingLogLikes(0.1 * c.samples[:, 0] ** 2)
    c.filter(c.samples[:, 1] > 1.0)
    assert c.numrows < s.numrows == 3001 and gu.relerr(c.means, means) > 1e-3
    s.needs_update = True  # the parent's statistics and density again, from ITS resident columns
    s.updateBaseStatistics()
    assert gu.relerr(s.means, means) < TOL_MOMENTS and gu.relerr(s.fullcov, cov) < TOL_MOMENTS
    assert np.max(np.abs(s.get1DDensity("x").P - dens)) < TOL_GRID
    assert np.array_equal(device_rows(s.ctx, 1), s.samples[:, 1])


def test_copy_with_settings():
    s = build("A")
    s.get1DDensity("x")
    c = s.copy(settings={"smooth_scale_1D": 0.3})
    fresh = build("A", settings={"smooth_scale_1D": 0.3})
    want = fresh.get1DDensity("x").P
    assert np.max(np.abs(c.get1DDensity("x").P - want)) < TOL_GRID
    assert s.smooth_scale_1D == -1.0 and np.max(np.abs(s.get1DDensity("x").P - want)) > 1e-3


def test_copy_after_2d_densities():
    """The parent has device-side state of its own by now (index columns, blocks of the batched call): none of it is
    copied, and the copy makes the same density from its own columns."""
    s = build("B")
    want = s.get2DDensity("x", "y").P.copy()
    c = s.copy()
    assert c._idx_cols == {} and c._twin is None and c._pending_results is None
    assert np.max(np.abs(c.get2DDensity("x", "y").P - want)) < TOL_GRID
    assert np.max(np.abs(s.get2DDensity("x", "y").P - want)) < TOL_GRID


def test_copy_of_chains_keeps_gelman_rubin():
    s = build("MC")
    want = s.getGelmanRubin()
    c = s.copy()
    assert c._chain_stats_cache == {} and np.array_equal(c.chain_offsets, s.chain_offsets)
    assert abs(c.getGelmanRubin() - want) <= TOL_SCALAR * want


# ---- combined sample sets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(cc.COMBINED))
def test_combined(gold, case):
    from getdist_amd.mcsamples import MCSamples

    got = cc.combine(MCSamples, case)
    key = "comb/" + case
    assert got.paramNames.list() == gold[key + "/names"].tolist()
    assert np.array_equal(got.weights, cc.shared(gold, key + "/weights"))
    assert np.array_equal(device_rows(got.ctx, -2), got.weights)
    assert gu.relerr(got.means, gold[key + "/means"]) < TOL_MOMENTS
    assert gu.relerr(got.fullcov, gold[key + "/cov"]) < TOL_MOMENTS
    d = got.get1DDensity("x")
    assert np.max(np.abs(d.P - gold[key + "/x_P"])) < TOL_GRID
    assert np.allclose([d.x[0], d.x[-1]], gold[key + "/x_x0x1"], rtol=1e-13, atol=0)
    check_limits(got.getMargeStats().parWithName("x"), gold[key + "/x_lims"], gold[key + "/x_meanerr"])


# ---- small queries -------------------------------------------------------------------------------------------------------
def test_queries(gold):
    a = build("A")
    w, U = a.getSignalToNoise(cc.SN_PARAMS, noise=cc.NOISE)
    assert np.max(np.abs(w - gold["A/sn_w"]) / np.abs(gold["A/sn_w"])) < TOL_SCALAR
    assert np.max(np.abs(cc.sign_fixed(U) - gold["A/sn_U"])) < TOL_SCALAR * np.max(np.abs(gold["A/sn_U"]))
    only = a.getSignalToNoise(cc.SN_PARAMS, noise=cc.NOISE, eigs_only=True)
    assert np.max(np.abs(only - gold["A/sn_w_only"]) / np.abs(gold["A/sn_w_only"])) < TOL_SCALAR

    b = a.getBounds()
    assert b.names == gold["A/bounds/names"].tolist()
    assert b.lower == dict(zip(gold["A/bounds/lower/keys"].tolist(), gold["A/bounds/lower/values"].tolist())) == {"x": 0.0}
    assert b.upper == {} and gold["A/bounds/upper/keys"].size == 0

    assert a.getCorrelatedVariable2DPlots(3) == gold["A/corr_pairs_3"].tolist()
    assert a.getCorrelatedVariable2DPlots(12, nparam=2) == gold["A/corr_pairs_12_2"].tolist()

    counts, numbers = cc.summary_numbers(a.getNumSampleSummaryText())
    want_counts, want = cc.summary_numbers(str(gold["A/summary"]))
    assert counts == want_counts == [3001, 4]
    assert np.max(np.abs(numbers - want) / want) < TOL_SCALAR, (numbers, want)

    assert a.getParamBestFitDict(best_sample=True) == a.getParamSampleDict(int(np.argmin(a.loglikes)))


# ---- lifetime: nothing of the copy is borrowed from the parent (keep this the LAST test of the file) ------------------------
def test_copy_outlives_the_parent_context():
    s = build("A")
    means, dens = s.means.copy(), s.get1DDensity("x").P.copy()
    c = s.copy()
    s.ctx.close()
    c.needs_update = True  # statistics and density from the copy's own columns, the parent's being freed
    assert np.max(np.abs(c.get1DDensity("x").P - dens)) < TOL_GRID
    assert gu.relerr(c.getMeans(), means) < TOL_MOMENTS
    assert np.array_equal(device_rows(c.ctx, 0), s.samples[:, 0])
