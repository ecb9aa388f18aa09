"""GPU tests of the routes of stats.hip that the other files do not reach, through the context's public calls, against
numpy in double precision: gd_cov in every slab configuration, in the two-pass slab form and on the tile route, the
single-lag kernel of the Gaussian-kernel lag sums (more lags than one multi-lag launch takes), and the 2D lag sums."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_COV, LO, HI = 3001, 1, 3000  # an odd first row: the ragged head; 2999 rows: 12 to 24 blocks of the slab kernel
N_COLS = 230
# the last width of each slab configuration, one first width, the two-pass slab (208) and the tile route with four tiles
COV_WIDTHS = [1, 31, 32, 47, 63, 79, 95, 111, 143, 191, 207, 208, 209]
N_LAG = 5001


@pytest.fixture(scope="module")
def ctx():
    from getdist_amd._lib import Context

    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cov_cases():
    """{weighted: (samples, weights or None, reference means, covariance, min / max of all columns over the row range)}"""
    r = np.random.default_rng(2024)
    z = r.standard_normal((N_COV, N_COLS))
    mix = np.eye(N_COLS) + 0.3 * np.diag(np.ones(N_COLS - 1), 1) + 0.1 * np.diag(np.ones(N_COLS - 7), 7)
    s = (z @ mix) * r.uniform(0.5, 2.0, N_COLS) + r.uniform(-5.0, 5.0, N_COLS)
    out = {}
    for weighted in (False, True):
        w = r.random(N_COV) + 0.25 if weighted else None
        ws, ss = (w[LO:HI] if weighted else np.ones(HI - LO)), s[LO:HI]
        means = ws.dot(ss) / ws.sum()
        d = ss - means
        cov = (d * ws[:, None]).T @ d / ws.sum()
        mm = np.stack([ss.min(axis=0), ss.max(axis=0)], axis=1)
        for a in (s, means, cov, mm):
            a.setflags(write=False)
        out[weighted] = (s, w, means, cov, mm, ws.sum())
    return out


def _check_cov(ctx, case, m):
    s, w, means, cov, mm, norm = case
    cols = np.random.default_rng(m).permutation(N_COLS)[:m]  # shuffled, not contiguous
    ctx.upload(s, w)
    got_means, got_cov, got_norm, got_mm = ctx.cov(cols=cols, lo=LO, hi=HI, minmax=True)
    assert abs(got_norm - norm) <= 1e-12 * norm
    assert np.allclose(got_means, means[cols], rtol=1e-12, atol=1e-14)
    assert np.allclose(got_cov, cov[np.ix_(cols, cols)], rtol=1e-11, atol=1e-13)
    assert np.array_equal(got_cov, got_cov.T)
    assert np.array_equal(got_mm, mm[cols])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", COV_WIDTHS)
def test_cov_on_every_route(ctx, cov_cases, m, weighted):
    _check_cov(ctx, cov_cases[weighted], m)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", [m for m in COV_WIDTHS if m <= 207])
def test_cov_two_pass_slab_in_every_configuration(ctx, cov_cases, m, weighted, monkeypatch):
    monkeypatch.setenv("GDHIP_COV_TWOPASS", "1")
    _check_cov(ctx, cov_cases[weighted], m)


@pytest.fixture(scope="module")
def lag_cases():
    r = np.random.default_rng(77)
    x = np.cumsum(r.standard_normal((N_LAG, 2)), axis=0) * 0.05 + r.standard_normal((N_LAG, 2))
    return {False: (x, None, np.ones(N_LAG)), True: (x, r.random(N_LAG) + 0.25, None)}


@pytest.mark.parametrize("weighted", [False, True])
def test_lag_sums_of_nine_lags_take_the_single_lag_kernel(ctx, lag_cases, weighted):
    x, w, ones = lag_cases[weighted]
    ww = w if weighted else ones
    ctx.upload(x, w)
    lags = np.array([1, 2, 3, 7, 50, 1000, N_LAG // 2, N_LAG // 2 + 4, N_LAG - 2], dtype=np.int64)
    c = np.array([1.0 / (4 * 0.3**2), 0.8])
    ref = np.array([[np.dot(np.exp(-((x[:-k, j] - x[k:, j]) ** 2) * c[j]) * ww[:-k], ww[k:]) for k in lags] for j in range(2)])
    got = ctx.kde_lag_sums_batch([0, 1], c, lags)
    assert np.allclose(got, ref, rtol=1e-12), np.abs(got / ref - 1).max()


@pytest.mark.parametrize("weighted", [False, True])
def test_lag_sums_2d(ctx, lag_cases, weighted):
    x, w, ones = lag_cases[weighted]
    ww = w if weighted else ones
    ctx.upload(x, w)
    lags = np.array([1, 2, 7, N_LAG // 2, N_LAG // 2 + 4], dtype=np.int64)
    k00, k01s, k11 = 2.5, -1.2, 1.75  # K00, K01 + K10, K11 of inv(cov) / h^2
    ref = []
    for k in lags:
        dx, dy = x[:-k, 1] - x[k:, 1], x[:-k, 0] - x[k:, 0]
        ref.append(np.dot(np.exp(-(dx * (k00 * dx) + dx * (k01s * dy) + dy * (k11 * dy)) / 4.0) * ww[:-k], ww[k:]))
    got = ctx.kde_lag_sums_2d(1, 0, [k00, k01s, k11], lags)
    assert np.allclose(got, ref, rtol=1e-12), np.abs(got / np.array(ref) - 1).max()
