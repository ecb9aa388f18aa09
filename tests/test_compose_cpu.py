"""CPU tier of MCSamples.copy / copy.deepcopy, getCombinedSamplesWithSamples and the look-ups and small queries around them
(getParamSampleDict, getParamBestFitDict, getBounds, getCorrelatedVariable2DPlots, getNumSampleSummaryText,
getSignalToNoise, setParams / getParams, updateRenames): the host logic over the numpy double of the context, held to the
reference's outputs in tests/golden/compose.npz."""

import copy
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_cases as cc  # noqa: E402
from fake_ctx import FakeContext  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


def build(fx, **kw):
    from getdist_amd.mcsamples import MCSamples

    return cc.build(MCSamples, fx, _context_factory=FakeContext, **kw)


@pytest.fixture(scope="module")
def A():
    return build("A")


def as_dict(gold, key):
    return dict(zip(gold[key + "/keys"].tolist(), gold[key + "/values"].tolist()))


def same_dict(got, want):
    return list(got) == list(want) and all(float(got[k]) == want[k] for k in want)


# ---- combined sample sets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(cc.COMBINED))
def test_combined_arrays(gold, case):
    from getdist_amd.mcsamples import MCSamples

    got = cc.combine(MCSamples, case, _context_factory=FakeContext)
    key = "comb/" + case
    assert isinstance(got, MCSamples) and isinstance(got.ctx, FakeContext)
    assert got.paramNames.list() == gold[key + "/names"].tolist()
    assert got.paramNames.labels() == gold[key + "/labels"].tolist()
    assert [p.isDerived for p in got.paramNames.names] == gold[key + "/derived"].tolist()
    assert np.array_equal(got.samples, cc.shared(gold, key + "/samples"))
    assert np.array_equal(got.weights, cc.shared(gold, key + "/weights"))
    assert (got.loglikes is not None) == bool(gold[key + "/has_loglikes"])
    if got.loglikes is not None:
        assert np.array_equal(got.loglikes, cc.shared(gold, key + "/loglikes"))
    assert got.chain_offsets is None and got.ignore_rows == 0
    if case == "FX":
        assert got.ranges.fixedValueDict() == as_dict(gold, key + "/fixed") == {"c": cc.FIXED_VALUE}


def test_combined_takes_ranges_and_settings_as_copies():
    first, second = build("A", settings={"smooth_scale_1D": 0.4, "contours": [0.5, 0.9]}), build("B")
    got = first.getCombinedSamplesWithSamples(second)
    assert got.smooth_scale_1D == 0.4 and got.contours == [0.5, 0.9] and got.contours is not first.contours
    assert got.ranges is not first.ranges and got.ranges.lower == first.ranges.lower
    assert second.smooth_scale_1D == -1.0
    assert got.numrows == first.numrows + second.numrows


# ---- look-ups ------------------------------------------------------------------------------------------------------
def test_param_sample_dicts(gold, A):
    assert same_dict(A.getParamSampleDict(5), as_dict(gold, "A/sample5"))
    assert same_dict(A.getParamSampleDict(5, want_derived=False), as_dict(gold, "A/sample5_noderived"))
    fxa = build("FXA")
    assert same_dict(fxa.getParamSampleDict(5, want_fixed=True), as_dict(gold, "FXA/sample5_fixed"))
    assert same_dict(fxa.getParamSampleDict(5, want_fixed=False), as_dict(gold, "FXA/sample5_nofixed"))
    assert build("U").getParamSampleDict(3)["weight"] == 1.0


def test_best_fit_sample_dict(gold, A):
    assert same_dict(A.getParamBestFitDict(best_sample=True), as_dict(gold, "A/bestfit_sample"))


def test_look_up_errors(A):
    nl = build("NL")
    with pytest.raises(TypeError):
        nl.getParamSampleDict(0)
    with pytest.raises(ValueError, match="No likelihoods in samples"):
        nl.getParamBestFitDict(best_sample=True)
    with pytest.raises(ValueError, match="best_fit_sample is only maximum posterior"):
        A.getParamBestFitDict(best_sample=True, max_posterior=False)
    with pytest.raises(NotImplementedError, match="best-fit files are outside the accelerated path"):
        A.getParamBestFitDict()
    with pytest.raises(NotImplementedError, match="best-fit files are outside the accelerated path"):
        A.getMargeStats(include_bestfit=True)


def test_set_params_dotted_names():
    from getdist_amd.chains import ParSamples
    from getdist_amd.mcsamples import MCSamples

    s = np.random.default_rng(5).standard_normal((40, 5))
    names = ["aa", "aa.bb", "plain", "m.n.o", "aa.cc.dd"]
    mc = MCSamples(samples=s, names=names, _context_factory=FakeContext)
    p = mc.getParams()
    assert isinstance(p, ParSamples) and isinstance(p.aa, ParSamples) and isinstance(p.m.n, ParSamples)
    assert np.array_equal(p.aa.value, s[:, 0])  # aa is a parameter AND the head of dotted names: .value
    assert np.array_equal(p.aa.bb, s[:, 1])
    assert np.array_equal(p.plain, s[:, 2])
    assert np.array_equal(p.m.n.o, s[:, 3])
    assert np.array_equal(p.aa.cc.dd, s[:, 4])
    mine = types.SimpleNamespace(other=1)
    assert mc.setParams(mine) is mine and mine.other == 1 and np.array_equal(mine.plain, s[:, 2])
    # the same whichever of the two comes first in the parameter list
    rev = MCSamples(samples=s[:, :2], names=["aa.bb", "aa"], _context_factory=FakeContext).getParams()
    assert np.array_equal(rev.aa.value, s[:, 1]) and np.array_equal(rev.aa.bb, s[:, 0])


def test_get_params_plain_names_unchanged(A):
    p = A.getParams()
    for j, nm in enumerate(A.paramNames.list()):
        assert np.array_equal(getattr(p, nm), A.samples[:, j])
    assert sorted(vars(p)) == sorted(A.paramNames.list())


def test_update_renames():
    mc = build("B")
    mc.updateRenames({"x": "ex", "q": ["qu", "kew"], "nobody": "nothing"})
    assert mc.getRenames() == {"x": ["ex"], "q": ["qu", "kew"]}
    mc.updateRenames({"ex": "chi", "kew": ["qq"]})  # through a name that is already an alternative
    assert set(mc.getRenames()["x"]) == {"ex", "chi"} and set(mc.getRenames()["q"]) == {"qu", "kew", "qq"}
    assert mc.paramNames.parWithName("chi").name == "x" and mc._col("z") == 0
    assert "y" not in mc.getRenames() and "z" not in mc.getRenames()


# ---- small queries -------------------------------------------------------------------------------------------------
def test_bounds(gold, A):
    b = build("A").getBounds()  # (a fresh object: nothing but getBounds itself has run the range logic)
    assert b.names == gold["A/bounds/names"].tolist()
    assert b.lower == as_dict(gold, "A/bounds/lower") and b.upper == as_dict(gold, "A/bounds/upper")
    assert b.lower == {"x": 0.0}
    far = build("A")
    far.setRanges({"y": (-1000.0, 1000.0)})  # a range the samples stay far from is no bound
    assert far.getBounds().lower == {"x": 0.0} and far.getBounds().upper == {}


def test_correlated_pairs(gold, A):
    assert A.getCorrelatedVariable2DPlots(3) == gold["A/corr_pairs_3"].tolist()
    assert A.getCorrelatedVariable2DPlots(12, nparam=2) == gold["A/corr_pairs_12_2"].tolist()
    assert A.getCorrelatedVariable2DPlots() == gold["A/corr_pairs_3"].tolist()  # 3 non-derived parameters: 3 pairs


@pytest.mark.parametrize("fx", ["B", "U"])
def test_summary_text(gold, fx):
    mc = build(fx)
    assert mc.indep_thin == 0
    assert mc.getNumSampleSummaryText() == str(gold[fx + "/summary"])


def test_summary_text_indep_thin_line():
    mc = build("MC")
    assert mc.indep_thin == 0 and "Approx indep samples" not in mc.getNumSampleSummaryText()
    mc.getCorrLengths()
    assert mc.indep_thin != 0
    lines = mc.getNumSampleSummaryText().splitlines()
    assert len(lines) == 4 and lines[1] == "Approx indep samples (N/corr length): %s" % round(mc.norm / mc.indep_thin)


def test_signal_to_noise(gold, A):
    from getdist_amd import chains

    w, U = A.getSignalToNoise(cc.SN_PARAMS, noise=cc.NOISE)
    assert np.allclose(w, gold["A/sn_w"], rtol=1e-9, atol=0)
    assert np.allclose(cc.sign_fixed(U), gold["A/sn_U"], rtol=0, atol=1e-9 * np.max(np.abs(gold["A/sn_U"])))
    only = A.getSignalToNoise(cc.SN_PARAMS, noise=cc.NOISE, eigs_only=True)
    assert np.allclose(only, gold["A/sn_w_only"], rtol=1e-9, atol=0)
    C = A.cov(cc.SN_PARAMS)
    R = np.linalg.inv(np.linalg.cholesky(cc.NOISE))
    assert np.array_equal(chains.getSignalToNoise(C, R=R, eigs_only=True), chains.getSignalToNoise(C, noise=cc.NOISE, eigs_only=True))
    with pytest.raises(chains.WeightedSampleError):
        chains.getSignalToNoise(C)


# ---- copy ----------------------------------------------------------------------------------------------------------
HOST_ARRAYS = ("samples", "weights", "loglikes", "means", "vars", "sddev", "fullcov", "_col_min", "_col_max")


class NotToBeCopied:
    """Stands for device buffers and futures among the parent's state: copying one would free device memory twice."""

    def __deepcopy__(self, memo):
        raise AssertionError("state bound to the parent's context or threads was deep-copied")


def check_copy(s, c):
    assert type(c) is type(s) and c is not s
    assert c.ctx is not s.ctx and isinstance(c.ctx, FakeContext)
    for att in HOST_ARRAYS:
        a, b = getattr(s, att), getattr(c, att)
        if a is None:
            assert b is None, att
        else:
            assert np.array_equal(a, b) and not np.shares_memory(a, b), att
    assert (s.chain_offsets is None) == (c.chain_offsets is None)
    assert c.norm == s.norm and c.numrows == s.numrows and c.n == s.n and c.index == s.index
    assert c.paramNames is not s.paramNames and c.paramNames.list() == s.paramNames.list()
    for p, q in zip(s.paramNames.names, c.paramNames.names):
        assert p is not q
        for att in ("label", "isDerived", "limmin", "limmax", "has_limits_bot", "has_limits_top", "N_eff_kde"):
            assert getattr(p, att) == getattr(q, att), (p.name, att)
        if getattr(p, "_ranges_done", False):
            assert (q.range_min, q.range_max, q.has_limits) == (p.range_min, p.range_max, p.has_limits)
    assert c.ranges is not s.ranges and c.ranges.lower == s.ranges.lower and c.ranges.upper == s.ranges.upper
    assert c.contours == s.contours and c.contours is not s.contours
    assert sorted(c.density1D) == sorted(s.density1D)
    for nm in s.density1D:
        assert np.array_equal(c.density1D[nm].P, s.density1D[nm].P) and not np.shares_memory(c.density1D[nm].P, s.density1D[nm].P)
    # nothing that belongs to the parent's contexts and threads
    assert c._twin is None and c._helper_exec is None and c._lane_exec is None and c._pending_results is None
    assert c._idx_cols == {} and c._chain_stats_cache == {} and c._loglikes_col is None
    assert c.ctx.N == s.ctx.N and c.ctx.n == s.ctx.n and not np.shares_memory(c.ctx.s, s.ctx.s)


@pytest.mark.parametrize("how", ["copy", "deepcopy"])
@pytest.mark.parametrize("fx", ["A", "U", "MC", "ONE"])
def test_copy_is_equal_and_independent(fx, how):
    s = build(fx)
    s.get1DDensity("x")  # a cached density, ranges and N_eff of x
    if fx == "MC":
        s.getGelmanRubin()  # fills _chain_stats_cache
    s._idx_cols["sentinel"] = s._chain_stats_cache["sentinel"] = s._lag_prefetch = s._parked = NotToBeCopied()
    c = s.copy() if how == "copy" else copy.deepcopy(s)
    del s._idx_cols["sentinel"], s._chain_stats_cache["sentinel"]
    s._lag_prefetch = s._parked = None
    assert c._lag_prefetch is None and c._parked is None
    check_copy(s, c)
    if fx == "MC":
        assert np.array_equal(c.chain_offsets, s.chain_offsets) and not np.shares_memory(c.chain_offsets, s.chain_offsets)
        assert c.getGelmanRubin() == s.getGelmanRubin()
    assert np.array_equal(c.get1DDensity("x").P, s.get1DDensity("x").P)


def test_copy_label_and_settings():
    s = build("A", settings={"smooth_scale_1D": 0.5})
    s.label = "parent"
    s.needs_update = False
    c = s.copy(label="child", settings={"smooth_scale_1D": 0.3, "fine_bins": 512})
    assert (c.label, s.label) == ("child", "parent")
    assert (c.smooth_scale_1D, c.fine_bins, c.needs_update) == (0.3, 512, True)
    assert (s.smooth_scale_1D, s.fine_bins, s.needs_update) == (0.5, 1024, False)
    assert s.copy().label == "parent" and s.copy().needs_update is False
    fresh = build("A", settings={"smooth_scale_1D": 0.3, "fine_bins": 512})
    assert np.array_equal(c.get1DDensity("x").P, fresh.get1DDensity("x").P)


def test_mutating_the_copy_leaves_the_parent():
    s = build("A")
    rows, means, dens = s.numrows, s.means.copy(), s.get1DDensity("x").P.copy()
    c = s.copy()
    c.filter(c.samples[:, 1] > 1.0)
    c.reweightAddingLogLikes(0.1 * c.samples[:, 0] ** 2)
    assert c.numrows < rows and not np.allclose(c.means, means)
    assert s.numrows == rows and s.ctx.N == rows and np.array_equal(s.means, means)
    s.needs_update = True
    assert np.array_equal(s.get1DDensity("x").P, dens) and np.array_equal(s.means, means)


def test_copy_of_a_column_share_is_refused(A):
    from getdist_amd.mcsamples import MCSamplesError

    s = build("ONE")
    s._column_share = object()
    with pytest.raises(MCSamplesError):
        s.copy()
    with pytest.raises(MCSamplesError):
        copy.deepcopy(s)


# ---- the native entry point behind copy ------------------------------------------------------------------------------
def test_clone_samples_is_exported_and_bound():
    from getdist_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_native()
    lib = _lib.load_library()
    assert hasattr(lib, "gd_clone_samples")
    restype, argtypes = _lib.SIGNATURES["gd_clone_samples"]
    assert restype is _lib.C.c_int and len(argtypes) == 2
    assert callable(getattr(_lib.Context, "clone_samples"))
    header = open(os.path.join(cc.ROOT, "include", "gdhip.h")).read()
    assert "int gd_clone_samples(gd_ctx* dst, gd_ctx* src);" in header
