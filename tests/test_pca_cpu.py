"""CPU tier of MCSamples.PCA: the host logic (maps, text, eigen-decomposition, normalisation, n_best_only, file output) runs
over a numpy double of Context.pca_corr / pca_project and is held to the reference's texts in tests/golden/pca.npz."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_cases  # noqa: E402
from fake_ctx import FakeContext  # noqa: E402


class PCAContext(FakeContext):
    """FakeContext + the vectorised numpy restatement of gd_pca_corr / gd_pca_project (sample weights always)."""

    calls = {"corr": 0, "project": 0}

    def _sample_w(self):
        return self.w

    def pca_corr(self, cols, maps):
        type(self).calls["corr"] += 1
        return pca_cases.np_corr(self.s[:, :self.n], self._sample_w(), list(cols), list(maps))

    def pca_project(self, cols, maps, mean, sd, U, doexp, all_means, all_sd):
        type(self).calls["project"] += 1
        return pca_cases.np_project(self.s[:, :self.n], self._sample_w(), list(cols), list(maps), np.asarray(mean),
                                    np.asarray(sd), np.asarray(U), doexp, np.asarray(all_means), np.asarray(all_sd))


@pytest.fixture(scope="module")
def gold():
    return pca_cases.load_golden()


@pytest.fixture(scope="module")
def samples():
    from getdist_amd.mcsamples import MCSamples

    return {fx: pca_cases.build(MCSamples, fx, _context_factory=PCAContext) for fx in pca_cases.CASES}


def test_pca_entries_exported_and_bound():
    from getdist_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_native()
    lib = _lib.load_library()
    for name in ("gd_pca_corr", "gd_pca_project"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.Context, "pca_corr") and hasattr(_lib.Context, "pca_project")


def test_golden_specs_match_cases(gold):
    for fx, i in pca_cases.all_cases():
        assert str(gold[pca_cases.case_key(fx, i) + "/spec"]) == pca_cases.case_spec(fx, i)


@pytest.mark.parametrize("fx,i", list(pca_cases.all_cases()))
def test_pca_text_matches_reference(samples, gold, fx, i):
    key = pca_cases.case_key(fx, i)
    r = samples[fx].PCA(**pca_cases.CASES[fx][i])
    kind = str(gold[key + "/kind"])
    if kind == "str":
        assert isinstance(r, str)
    else:
        assert isinstance(r, list) and len(r) == int(kind[4:])
    bad = pca_cases.text_mismatches(pca_cases.as_text(r), str(gold[key + "/text"]))
    assert not bad, "\n".join(bad[:5])


def test_n_best_only_types(samples):
    mc = samples["powerlaw_unit"]
    one = mc.PCA(["omegam", "sigma8", "H0"], n_best_only=1)
    two = mc.PCA(["omegam", "sigma8", "H0"], n_best_only=2)
    full = mc.PCA(["omegam", "sigma8", "H0"])
    assert isinstance(one, str) and one.startswith("PC1 (e-value:")
    assert isinstance(two, list) and len(two) == 2 and two[0] == one
    assert isinstance(full, str) and full.startswith("PCA for parameters:\n") and one in full and two[1] in full


def test_write_data_to_file(samples, tmp_path):
    mc = samples["mixed_int"]
    target = tmp_path / "explicit.txt"
    text = mc.PCA(["a", "neg", "b"], writeDataToFile=True, filename=str(target))
    assert target.read_text(encoding="utf-8") == text
    assert mc.rootdirname == ""
    mc.rootdirname = str(tmp_path / "chain_root")
    try:
        best = mc.PCA(["a", "neg", "b"], writeDataToFile=True, n_best_only=1)
    finally:
        mc.rootdirname = ""
    assert (tmp_path / "chain_root.PCA").read_text(encoding="utf-8") == text
    assert isinstance(best, str) and best in text


def test_log_of_zero_crossing_column_raises_linalg_error(samples):
    """L on a column that crosses zero: NaN in the correlation matrix, and eig raises like the reference."""
    with pytest.raises(np.linalg.LinAlgError):
        samples["mixed_int"].PCA(["a", "x"], param_map="LL")


def test_par_name_and_label(samples):
    mc = samples["real_derived"]
    assert mc.parName(0) == "p" and mc.parName(3) == "pr" and mc.parName(3, starDerived=True) == "pr*"
    assert mc.parName(0, starDerived=True) == "p"
    assert mc.parLabel(3) == "p r" and mc.parLabel("q") == "q"


def test_device_entries_do_the_work(samples):
    before = dict(PCAContext.calls)
    samples["powerlaw_unit"].PCA(["omegam", "sigma8"])
    assert PCAContext.calls["corr"] == before["corr"] + 1 and PCAContext.calls["project"] == before["project"] + 1


def test_column_share_context_refuses():
    from getdist_amd.mcsamples import MCSamples

    mc = pca_cases.build(MCSamples, "powerlaw_unit", _context_factory=PCAContext)
    mc._column_share = object()  # a context that holds only its rank's block of columns
    with pytest.raises(NotImplementedError):
        mc.PCA(["omegam", "sigma8"])


def _reference_steps(f, cols, maps, u_rows=None):
    """Steps 1-5 of the reference written out per column and per row (small N): the loops of mcsamples.py:760-870."""
    X = f["samples"][:, cols].astype(float).copy()
    w = np.ones(len(X)) if f["weights"] is None else f["weights"]
    norm = np.sum(w)
    n = len(cols)
    mean, sd = np.zeros(n), np.zeros(n)
    for i in range(n):
        if maps[i] == 1:
            X[:, i] = np.log(X[:, i])
        elif maps[i] == 2:
            X[:, i] = np.log(-1.0 * X[:, i])
        mean[i] = np.dot(w, X[:, i]) / norm
        X[:, i] -= mean[i]
        sd[i] = np.sqrt(np.dot(w, X[:, i] ** 2) / norm)
        if sd[i] != 0:
            X[:, i] /= sd[i]
    C = np.ones((n, n))
    for i in range(n):
        for j in range(i):
            C[j][i] = C[i][j] = np.dot(w, X[:, i] * X[:, j]) / norm
    return X, w, norm, mean, sd, C


def test_numpy_restatement_pinned_to_per_row_loops():
    """The vectorised restatement the GPU tests use at large N equals the reference's loops (steps 1-5) on a fixture."""
    f = pca_cases.fixtures()["real_derived"]
    cols, maps = [0, 1, 2], [1, 0, 1]
    Z, w, norm, mean, sd, C = _reference_steps(f, cols, maps)
    m2, s2, C2 = pca_cases.np_corr(f["samples"], f["weights"], cols, maps)
    np.testing.assert_allclose(m2, mean, rtol=1e-12)
    np.testing.assert_allclose(s2, sd, rtol=1e-12)
    np.testing.assert_allclose(C2, C, rtol=1e-11, atol=1e-14)
    evals, evects = np.linalg.eig(C)
    u = np.transpose(evects[:, evals.argsort()])
    for i in range(3):
        k = np.abs(u[i, :]).argmax()
        u[i, :] = u[i, :] / u[i, k] * sd[k]
    P = np.array([np.exp(np.dot(u, Z[r, :])) for r in range(len(Z))])  # the reference's per-row loop
    newmean = np.array([np.dot(w, P[:, i]) / norm for i in range(3)])
    newsd = np.array([np.sqrt(np.dot(w, (P[:, i] - newmean[i]) ** 2) / norm) for i in range(3)])
    Q = (P - newmean) / newsd
    S = f["samples"]
    means = np.array([np.dot(w, S[:, j]) / norm for j in range(S.shape[1])])
    sddev = np.sqrt(np.array([np.dot(w, (S[:, j] - means[j]) ** 2) / norm for j in range(S.shape[1])]))
    pcpc = np.array([[np.dot(w, Q[:, i] * Q[:, j]) / norm for j in range(3)] for i in range(3)])
    pcpar = np.array([[np.sum(w * Q[:, i] * (S[:, j] - means[j]) / sddev[j]) / norm for j in range(S.shape[1])]
                      for i in range(3)])
    r = pca_cases.np_project(S, w, cols, maps, mean, sd, u, True, means, sddev, chunk=7000)
    np.testing.assert_allclose(r[0], newmean, rtol=1e-12)
    np.testing.assert_allclose(r[1], newsd, rtol=1e-11)
    np.testing.assert_allclose(r[2], pcpc, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(r[3], pcpar, rtol=1e-10, atol=1e-13)
    # chunking does not change the restatement beyond rounding
    m3, s3, C3 = pca_cases.np_corr(f["samples"], f["weights"], cols, maps, chunk=3000)
    np.testing.assert_allclose(C3, C2, rtol=1e-12, atol=1e-15)


def test_text_rule():
    assert not pca_cases.text_mismatches("PC 1   0.123  -0.000\n", "PC 1   0.124   0.000\n")
    assert pca_cases.text_mismatches("PC 1   0.121\n", "PC 1   0.123\n")
    assert pca_cases.text_mismatches("PC 1   0.123\n", "PC 3   0.123\n")
    assert pca_cases.text_mismatches("a\nb", "a\nb\n")
    assert pca_cases.text_mismatches("[0.1]  (x/1.0)^{2.0}", "[0.1]  (y/1.0)^{2.0}")
