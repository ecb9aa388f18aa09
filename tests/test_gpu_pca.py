"""GPU tier of MCSamples.PCA: gd_pca_corr / gd_pca_project against the reference's texts (tests/golden/pca.npz) and, at
sizes where the reference is too slow, against the vectorised numpy restatement of steps 1-5 (tests/pca_cases.py)."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_cases  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = 1_000_000  # rows per chunk of the numpy restatement


def _mc(s, w=None, names=None, **kw):
    from getdist_amd.mcsamples import MCSamples

    return MCSamples(samples=s, weights=w, names=names or ["p%d" % i for i in range(s.shape[1])], **kw)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def _default_maps(mc, cols):
    return [0 if (mc._col_max[j] < 0 or mc._col_min[j] < (mc._col_max[j] - mc._col_min[j]) / 10) else 1 for j in cols]


def _eig_u(corr, sd):
    """eig, argsort and the largest-entry normalisation of mcsamples.py:800-833 (no conditional parameters)"""
    evals, evects = np.linalg.eig(corr)
    iso = evals.argsort()
    u = np.transpose(evects[:, iso])
    for i in range(len(u)):
        k = np.abs(u[i, :]).argmax()
        u[i, :] = u[i, :] / u[i, k] * sd[k]
    return evals[iso], u


def _separated(evals, gap=1e-6):
    ev = np.asarray(evals)
    ok = np.ones(len(ev), dtype=bool)
    for i in range(len(ev)):
        for j in (i - 1, i + 1):
            if 0 <= j < len(ev) and abs(ev[i] - ev[j]) <= gap * max(abs(ev[i]), 1e-300):
                ok[i] = False
    return ok


def _compare_full(mc, s, w, cols, maps, tol=1e-10):
    """Device steps 1-2 and 4-5 against the numpy restatement for the columns ``cols`` with ``maps``."""
    mean, sd, corr = mc.ctx.pca_corr(cols, maps)
    m2, s2, c2 = pca_cases.np_corr(s, w, cols, maps, chunk=CHUNK)
    # a mean is compared on the scale of its column's spread (zero-mean columns have means ~ sd / sqrt(N))
    assert np.max(np.abs(mean - m2) / np.maximum(np.abs(m2), s2)) < tol and _rel(sd, s2) < tol
    assert np.max(np.abs(corr - c2)) < tol
    ev, u = _eig_u(corr, sd)
    ev2, u2 = _eig_u(c2, s2)
    assert np.max(np.abs(ev - ev2)) < 10 * tol * max(1.0, np.max(np.abs(ev2)))
    sep = _separated(ev2)
    assert sep.sum() >= 1
    assert np.max(np.abs(u[sep] - u2[sep])) < 1e-6 * np.max(np.abs(u2[sep]))  # (eigenvectors: conditioned by the gaps)
    doexp = any(m != 0 for m in maps)
    # the projection with the same u on both sides
    r = mc.ctx.pca_project(cols, maps, mean, sd, u2, doexp, mc.means, mc.sddev)
    r2 = pca_cases.np_project(s, w, cols, maps, m2, s2, u2, doexp, mc.means, mc.sddev, chunk=CHUNK)
    assert np.max(np.abs(r[0] - r2[0]) / np.maximum(np.abs(r2[0]), r2[1])) < tol and _rel(r[1], r2[1]) < tol
    assert np.max(np.abs(r[2] - r2[2])) < tol and np.max(np.abs(r[3] - r2[3])) < tol


@pytest.fixture(scope="module")
def gold():
    return pca_cases.load_golden()


@pytest.fixture(scope="module")
def samples():
    from getdist_amd.mcsamples import MCSamples

    return {fx: pca_cases.build(MCSamples, fx) for fx in pca_cases.CASES}


@pytest.mark.parametrize("fx,i", list(pca_cases.all_cases()))
def test_pca_golden_on_device(samples, gold, fx, i):
    key = pca_cases.case_key(fx, i)
    r = samples[fx].PCA(**pca_cases.CASES[fx][i])
    assert (str(gold[key + "/kind"]) == "str") == isinstance(r, str)
    bad = pca_cases.text_mismatches(pca_cases.as_text(r), str(gold[key + "/text"]))
    assert not bad, "\n".join(bad[:5])


def test_device_entries_do_the_work(samples):
    mc = samples["powerlaw_unit"]
    calls = {"corr": 0, "project": 0}
    orig_c, orig_p = mc.ctx.pca_corr, mc.ctx.pca_project

    def corr(*a, **k):
        calls["corr"] += 1
        return orig_c(*a, **k)

    def project(*a, **k):
        calls["project"] += 1
        return orig_p(*a, **k)

    mc.ctx.pca_corr, mc.ctx.pca_project = corr, project
    try:
        mc.PCA(["omegam", "sigma8", "H0"])
    finally:
        del mc.ctx.pca_corr, mc.ctx.pca_project
    assert calls == {"corr": 1, "project": 1}


def test_c3_synth_full_size():
    from getdist_amd import synth

    s, w, names, _ = synth.config_c3(10_000_000, 50)
    mc = _mc(s, w, names)
    cols = list(range(50))
    _compare_full(mc, s, w, cols, _default_maps(mc, cols))


def test_lognormal_12_full_size():
    r = np.random.default_rng(7)
    N, n = 10_000_000, 12
    A = r.normal(size=(n, n)) * 0.3 + np.diag(np.linspace(1.0, 2.5, n))
    s = np.empty((N, n), order="F")
    for a in range(0, N, CHUNK):
        b = min(a + CHUNK, N)
        s[a:b] = np.exp(0.03 * r.standard_normal((b - a, n)) @ A.T + np.linspace(-1, 1, n))
    mc = _mc(s)
    cols = list(range(n))
    maps = _default_maps(mc, cols)
    assert all(m == 1 for m in maps)
    _compare_full(mc, s, None, cols, maps)
    text = mc.PCA(["p%d" % i for i in range(n)])
    assert text.count("PC") > 3 * n


def test_200_parameters():
    from getdist_amd import synth

    s, w, names, _ = synth.block_recipe(200, 200_000, weighted=True, stream=9)
    mc = _mc(s, w, names)
    cols = list(range(200))
    _compare_full(mc, s, w, cols, [0] * 200)
    assert mc.PCA(names, param_map="N" * 200, n_best_only=1).startswith("PC1 (e-value:")


def test_weights_correlated_with_x_two_pass():
    """Importance weights that grow steeply with x: the centred second pass keeps every digit (no provisional shift)."""
    r = np.random.default_rng(3)
    N = 2_000_000
    x = 1e4 + r.standard_normal(N)
    y = 0.5 * (x - 1e4) + r.standard_normal(N) + 50.0
    z = np.exp(0.01 * r.standard_normal(N)) * 3.0
    s = np.stack([x, y, z], axis=1)
    w = np.exp(4.0 * (x - 1e4) - 8.0)
    mc = _mc(s, w)
    _compare_full(mc, s, w, [0, 1, 2], [1, 0, 1])
    _compare_full(mc, s, w, [0, 1, 2], [0, 0, 0])


def test_reruns_bit_identical(samples):
    mc = samples["real_derived"]
    a = mc.ctx.pca_corr([0, 1, 2, 3], [1, 0, 1, 1])
    b = mc.ctx.pca_corr([0, 1, 2, 3], [1, 0, 1, 1])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    _, u = _eig_u(a[2], a[1])
    p = mc.ctx.pca_project([0, 1, 2, 3], [1, 0, 1, 1], a[0], a[1], u, True, mc.means, mc.sddev)
    q = mc.ctx.pca_project([0, 1, 2, 3], [1, 0, 1, 1], a[0], a[1], u, True, mc.means, mc.sddev)
    for x, y in zip(p, q):
        assert np.array_equal(x, y)
    assert mc.PCA(["p", "q", "r"]) == mc.PCA(["p", "q", "r"])


def test_sample_weights_while_aux_weights_selected(samples):
    mc = samples["mixed_int"]
    before = mc.ctx.pca_corr([0, 1, 3], [1, 2, 1])
    mc.ctx.aux_weights(np.ones(mc.numrows) * 3.0)
    mc.ctx.select_weights(1)
    try:
        during = mc.ctx.pca_corr([0, 1, 3], [1, 2, 1])
    finally:
        mc.ctx.select_weights(0)
    for x, y in zip(before, during):
        assert np.array_equal(x, y)


def test_after_mutators_equals_fresh():
    from getdist_amd.mcsamples import MCSamples

    f = pca_cases.fixtures()["mixed_int"]
    s, w = f["samples"], f["weights"]
    keep = s[:, 2] > -0.5
    mc = pca_cases.build(MCSamples, "mixed_int")
    mc.PCA(["a", "neg", "b"])  # device state of the full set first
    mc.filter(keep)
    fresh = MCSamples(samples=np.ascontiguousarray(s[keep]), weights=w[keep], names=f["names"], labels=f["labels"])
    assert mc.PCA(["a", "neg", "b"]) == fresh.PCA(["a", "neg", "b"])
    ll = 0.3 * (s[keep][:, 0] - 2.0) ** 2
    mc.reweightAddingLogLikes(ll)
    fresh2 = MCSamples(samples=np.ascontiguousarray(s[keep]), weights=w[keep] * np.exp(-(ll - ll.min())),
                       names=f["names"], labels=f["labels"])
    t1, t2 = mc.PCA(["a", "neg", "x"], param_map="LMN"), fresh2.PCA(["a", "neg", "x"], param_map="LMN")
    assert t1 == t2


def test_log_of_zero_crossing_column_raises_linalg_error(samples):
    mc = samples["mixed_int"]
    mean, sd, corr = mc.ctx.pca_corr([0, 2], [1, 1])
    assert np.isnan(mean[1]) and np.isnan(corr[0, 1])
    with pytest.raises(np.linalg.LinAlgError):
        mc.PCA(["a", "x"], param_map="LL")


def test_bad_arguments_return_status(samples):
    from getdist_amd._lib import GdhipError

    ctx = samples["mixed_int"].ctx
    with pytest.raises(GdhipError):
        ctx.pca_corr([], [])
    with pytest.raises(GdhipError):
        ctx.pca_corr([0, 99], [0, 0])
    with pytest.raises(GdhipError):
        ctx.pca_corr([0, 1], [0, 3])
    with pytest.raises(GdhipError):
        ctx.pca_project([0], [0], [0.0], [1.0], np.ones((1, 1)), False, np.zeros(99), np.ones(99))
