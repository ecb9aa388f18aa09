"""CPU tier of the raw N-D densities (getRawNDDensity / getRawNDDensityGridData / getRawNDDensities / DensityND): the host
orchestration runs over a numpy double of Context.histnd_batch and is held to the reference's outputs in
tests/golden/raw_nd.npz."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nd_cases  # noqa: E402
from fake_ctx import FakeContext  # noqa: E402


class NDContext(FakeContext):
    """FakeContext + a numpy double of gd_histnd_batch: the reference's index expression, np.bincount of the flat index
    (first axis fastest), np.minimum.at of the loglikes column."""

    histnd_calls = 0

    def histnd_batch(self, dims, cols, binmin, width, nb, want_h=True, want_likes=False, want_lmin=False, loglike_col=-1):
        type(self).histnd_calls += 1
        H, HL, L = [], [], []
        at = 0
        for d in dims:
            q = np.zeros(self.N, dtype=np.int64)
            for a in range(d):
                ix = ((self.s[:, cols[at + a]] - binmin[at + a]) / width[at + a] + 0.5).astype(int)
                if np.any((ix < 0) | (ix >= nb)):
                    raise ValueError("bin index outside the grid")
                q += ix * nb**a
            at += d
            M = nb**d
            if want_h:
                H.append(np.bincount(q, weights=self._w(), minlength=M).astype(float))
            if want_likes:
                HL.append(np.bincount(q, weights=self._like_w, minlength=M))
            if want_lmin:
                lm = np.full(M, np.inf)
                np.minimum.at(lm, q, self.s[:, loglike_col])
                L.append(lm)
        cat = lambda parts, want: np.concatenate(parts) if want else None  # noqa: E731
        return cat(H, want_h), cat(HL, want_likes), cat(L, want_lmin)


@pytest.fixture(scope="module")
def gold():
    return nd_cases.load_golden()


@pytest.fixture(scope="module")
def samples():
    return {fx: nd_cases.make_samples(fx, _context_factory=NDContext) for fx in nd_cases.CASES}


def test_histnd_entry_exported_and_bound():
    from getdist_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_native()
    lib = _lib.load_library()
    assert hasattr(lib, "gd_histnd_batch")
    assert "gd_histnd_batch" in _lib.SIGNATURES
    assert hasattr(_lib.Context, "histnd_batch")
    import getdist_amd

    assert getdist_amd.DensityND is getdist_amd.densities.DensityND


@pytest.mark.parametrize("fx,i", list(nd_cases.all_cases()))
def test_raw_nd_matches_reference(samples, gold, fx, i):
    d = nd_cases.run_case(samples[fx], fx, i)
    # the double adds in np.bincount's order: bit-equal P / contours for every weight kind
    nd_cases.check_case(d, gold, fx, i, exact=True)


def test_axis_order_and_edge_halving(samples):
    """P[i_{d-1}, ..., i_0] with the first parameter fastest; the faces of bounded parameters are halved before the max
    normalisation (mask axis i belongs to parv[::-1][i])."""
    mc = samples["c1_bounded_unit"]  # "d" (column 3) has a lower bound at 0; "a" (column 0) is unbounded
    d = mc.getRawNDDensity(["d", "a"])
    assert d.P.shape == (12, 12)
    assert np.array_equal(d.axes[0], d.xs[1]) and np.array_equal(d.axes[1], d.xs[0])
    names = mc.paramNames.names
    ix = []
    for j in (3, 0):
        fine_width, binmin, _ = mc._bin_edges(names[j], 12)
        ix.append(((mc.samples[:, j] - binmin) / fine_width + 0.5).astype(int))
    h = np.bincount(ix[0] + 12 * ix[1], minlength=144).astype(float).reshape(12, 12)  # [i_a, i_d]
    mask = np.ones((12, 12))
    mask[:, 0] /= 2  # the lower face of "d": axis 1
    want = h / mask
    np.testing.assert_array_equal(d.P, want / np.max(want))
    # without boundary correction nothing is halved
    d0 = mc.getRawNDDensity(["d", "a"], boundary_correction_order=-1)
    np.testing.assert_array_equal(d0.P, h / np.max(h))
    # a 1D raw grid is the 1D histogram of the reference's index rule
    d1 = mc.getRawNDDensity(["a"], num_bins_ND=9)
    fine_width, binmin, _ = mc._bin_edges(names[0], 9)
    h1 = np.bincount(((mc.samples[:, 0] - binmin) / fine_width + 0.5).astype(int), minlength=9).astype(float)
    np.testing.assert_array_equal(d1.P, h1 / h1.max())


def test_normalisations(samples):
    mc = samples["block10_real"]
    dmax = mc.getRawNDDensity(["p0", "p6"])
    assert np.max(dmax.P) == 1.0
    dint = mc.getRawNDDensity(["p0", "p6"], normalized=True)
    # the reference's DensityND.integrate: boundary classes weighted 1/2^k, no cell volume
    P = dmax.P
    k = (np.arange(12) == 0).astype(int) + (np.arange(12) == 11)
    wgt = 0.5 ** (k[:, None] + k[None, :])
    np.testing.assert_allclose(dint.P, P / np.sum(P * wgt), rtol=1e-14)
    assert dint.norm_integral() == pytest.approx(1.0, rel=1e-14)
    assert abs(dint.spacing - (dint.xs[0][1] - dint.xs[0][0]) * (dint.xs[1][1] - dint.xs[1][0])) == 0


def test_density_nd_class():
    from getdist_amd.densities import DensitiesError, DensityND

    xs = [np.linspace(0, 1, 4), np.linspace(-1, 1, 3), np.linspace(2, 3, 5)]
    d = DensityND(xs)
    assert d.dim == 3 and d.P.shape == (5, 3, 4)
    assert d.x is xs[0] and d.y is xs[1] and d.z is xs[2]
    assert d.spacing == (1 / 3) * 1.0 * 0.25
    d.setP(np.ones((5, 3, 4)))
    # corners 1/8, edges 1/4, faces 1/2, inside 1 -- counted per cell, no spacing
    k = [(np.arange(n) == 0).astype(int) + (np.arange(n) == n - 1) for n in (5, 3, 4)]
    want = np.sum(0.5 ** (k[0][:, None, None] + k[1][None, :, None] + k[2][None, None, :]))
    assert d.integrate(d.P) == want
    with pytest.raises(NotImplementedError):
        d.Prob([0.5, 0, 2.5])
    with pytest.raises(DensitiesError):
        DensityND(xs, P=np.ones((4, 3, 5)))
    with pytest.raises(DensitiesError):
        DensityND(xs).normalize("max")


def test_unknown_names_and_errors(samples):
    from getdist_amd.densities import DensitiesError
    from getdist_amd.mcsamples import MCSamplesError, SettingError

    mc = samples["c1_unit"]
    assert mc.getRawNDDensity(["a", "nope"]) is None
    assert mc.getRawNDDensityGridData(["nope"]) is None
    out = mc.getRawNDDensities([["a", "b"], ["zz"], ["c"]])
    assert out[1] is None and out[0].P.shape == (12, 12) and out[2].P.shape == (12,)
    with pytest.raises(NotImplementedError):
        mc.getRawNDDensityGridData(["a", "b"], writeDataToFile=True)
    with pytest.raises(SettingError):
        mc.getRawNDDensity(["a"], fine_bins_2D=10)
    # a flat 1D grid has no 99 % level inside 12 bins: the reference's DensitiesError
    with pytest.raises(DensitiesError):
        samples["shapes_int"].getRawNDDensityGridData(["s6"])
    # no loglikes: meanlikes / maxlikes refuse before any native call
    s, w, names, ranges, _, _ = nd_cases.fixtures()["c1_unit"]
    from getdist_amd.mcsamples import MCSamples

    bare = MCSamples(samples=s, weights=w, names=names, ranges=ranges, _context_factory=NDContext)
    before = NDContext.histnd_calls
    with pytest.raises(MCSamplesError):
        bare.getRawNDDensityGridData(["a", "b"], meanlikes=True)
    with pytest.raises(MCSamplesError):
        bare.getRawNDDensityGridData(["a", "b"], maxlikes=True)
    assert NDContext.histnd_calls == before


def test_batched_is_one_call_and_equals_single(samples):
    mc = samples["shapes_int"]
    lists = [["s0", "s1"], ["s4", "s5", "s6"], ["s2"], ["s0", "s1"]]
    before = NDContext.histnd_calls
    many = mc.getRawNDDensities(lists, meanlikes=True, maxlikes=True)
    assert NDContext.histnd_calls == before + 1
    for lst, d in zip(lists, many):
        one = mc.getRawNDDensityGridData(lst, meanlikes=True, maxlikes=True)
        for a in ("P", "likes", "maxlikes", "contours", "maxcontours"):
            assert np.array_equal(getattr(one, a), getattr(d, a)), (lst, a)


def test_num_bins_nd_setting(samples):
    mc = samples["c1_unit"]
    assert mc.num_bins_ND == 12
    mc.updateSettings({"num_bins_ND": 5})
    try:
        assert mc.getRawNDDensity(["a", "b"]).P.shape == (5, 5)
    finally:
        mc.updateSettings({"num_bins_ND": 12})
