"""GPU tier of the raw N-D densities: gd_histnd_batch through getRawNDDensity / getRawNDDensityGridData /
getRawNDDensities against the reference's outputs (tests/golden/raw_nd.npz) and against a vectorised numpy restatement
of the reference (index expression, np.bincount of the flat index, np.minimum.at of the loglikes) at full size."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nd_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return nd_cases.load_golden()


@pytest.fixture(scope="module")
def samples():
    return {fx: nd_cases.make_samples(fx) for fx in nd_cases.CASES}


@pytest.mark.parametrize("fx,i", list(nd_cases.all_cases()))
def test_raw_nd_golden_on_device(samples, gold, fx, i):
    d = nd_cases.run_case(samples[fx], fx, i)
    exact = nd_cases.fixtures()[fx][5] in ("unit", "int")
    nd_cases.check_case(d, gold, fx, i, exact=exact)


def test_nd_density_close_to_2d_density():
    """The reference's testNDDensity (getdist_test.py:167-179) with a numpy draw: unit 2D Gaussian truncated to [-2, 2]^2."""
    from getdist_amd.mcsamples import MCSamples

    for seed in (10, 11):
        r = np.random.default_rng(seed)
        z = r.standard_normal((1_400_000, 2))
        z = z[np.all(np.abs(z) <= 2, axis=1)][:1_000_000]
        assert len(z) == 1_000_000
        mc = MCSamples(samples=z, names=["x", "y"], ranges={"x": (-2, 2), "y": (-2, 2)})
        d2 = mc.get2DDensity("x", "y", fine_bins_2D=10, smooth_scale_2D=1, boundary_correction_order=1)
        dn = mc.getRawNDDensity(["x", "y"], num_bins_ND=10, boundary_correction_order=1)
        assert np.allclose(d2.P, dn.P, atol=1e-5), np.max(np.abs(d2.P - dn.P))


def _numpy_nd(mc, js, nb, weights, loglikes):
    """Reference restatement: H (bincount, first axis fastest, reshaped [i_{d-1}, ..., i_0]) and min loglike per bin."""
    q = np.zeros(mc.numrows, dtype=np.int64)
    for a, j in enumerate(js):
        fine_width, binmin, _ = mc._bin_edges(mc.paramNames.names[j], nb)
        q += ((mc.samples[:, j] - binmin) / fine_width + 0.5).astype(int) * nb**a
    M = nb ** len(js)
    H = np.bincount(q, weights=weights, minlength=M).reshape((nb,) * len(js))
    L = None
    if loglikes is not None:
        L = np.full(M, np.inf)
        np.minimum.at(L, q, loglikes)
        L = L.reshape((nb,) * len(js))
    return H, L


def _expected_P(mc, js, nb, H):
    from getdist_amd.mcsamples import _set_raw_edge_mask_nd

    parv = [mc.paramNames.names[j] for j in js]
    P = H.astype(float).copy()
    if any(p.has_limits for p in parv):
        mask = np.ones(P.shape)
        _set_raw_edge_mask_nd(parv, mask)
        P /= mask
    return P / np.max(P)


@pytest.fixture(scope="module")
def full():
    """N = 1e7 rows of six correlated columns (two bounded), loglikes, unit and real (Exp(1)) weights."""
    from getdist_amd.mcsamples import MCSamples

    N = 10_000_000
    r = np.random.default_rng(2024)
    z = r.standard_normal((N, 6))
    z[:, 1] += 0.6 * z[:, 0]
    z[:, 2] = np.abs(z[:, 2] + 0.3 * z[:, 1])
    z[:, 5] = np.where(z[:, 5] > 1.5, 3.0 - z[:, 5], z[:, 5])
    ll = 0.5 * np.sum(z[:, :3] ** 2, axis=1) + 0.1 * r.standard_normal(N)
    w = r.exponential(1.0, N)
    names = ["f%d" % i for i in range(6)]
    ranges = {"f2": (0.0, None), "f5": (None, 1.5)}
    unit = MCSamples(samples=z, loglikes=ll, names=names, ranges=ranges)
    real = MCSamples(samples=z, weights=w, loglikes=ll, names=names, ranges=ranges)
    return unit, real, w, ll


@pytest.mark.parametrize("js,nb", [((0, 2, 5), 12), ((0, 1, 2, 3, 5), 12), ((2, 4), 300)])
def test_full_size_against_numpy(full, js, nb):
    """3D at nb = 12 (LDS tier), 5D at nb = 12 (12^5 bins: global tier), 2D at nb = 300 (u16 index columns)."""
    unit, real, w, ll = full
    names = [unit.paramNames.names[j].name for j in js]
    du = unit.getRawNDDensityGridData(names, num_bins_ND=nb, maxlikes=True)
    H, L = _numpy_nd(unit, js, nb, None, ll)
    assert np.array_equal(du.P, _expected_P(unit, js, nb, H))
    bestfit = np.max(-ll)
    assert np.array_equal(du.maxlikes, np.exp(-bestfit - L))
    dr = real.getRawNDDensityGridData(names, num_bins_ND=nb, maxlikes=True, meanlikes=True)
    Hr, Lr = _numpy_nd(real, js, nb, w, ll)  # (the weighted parameter ranges give this sample set its own bin edges)
    Pr = _expected_P(real, js, nb, Hr)
    assert np.max(np.abs(dr.P - Pr)) <= 1e-10 * np.max(Pr)
    assert np.array_equal(dr.maxlikes, np.exp(-bestfit - Lr))
    HL, _ = _numpy_nd(real, js, nb, w * np.exp(real.mean_loglike - ll), None)
    HL = HL / np.max(HL)
    assert np.max(np.abs(dr.likes - HL)) <= 1e-10
    # real weights: a second call is bit-identical
    dr2 = real.getRawNDDensityGridData(names, num_bins_ND=nb, maxlikes=True, meanlikes=True)
    for a in ("P", "likes", "maxlikes", "contours", "maxcontours"):
        assert np.array_equal(getattr(dr, a), getattr(dr2, a)), a


def test_batched_equals_single_calls(full):
    unit, real, _, _ = full
    lists = [["f0", "f1", "f2"], ["f2", "f5"], ["f0", "f1", "f2"], ["f3"], ["f1", "f2", "f3", "f4"]]
    for mc in (unit, real):
        many = mc.getRawNDDensities(lists, meanlikes=True, maxlikes=True)
        for lst, d in zip(lists, many):
            one = mc.getRawNDDensityGridData(lst, meanlikes=True, maxlikes=True)
            for a in ("P", "likes", "maxlikes", "contours", "maxcontours"):
                assert np.array_equal(getattr(one, a), getattr(d, a)), (lst, a)


# (weights, outputs, nb on the LDS side, nb on the global side) of the 128-KB tier switch for 3D grids:
# counts 4 bytes per bin (32^3 = 32768 | 33^3), fixed point 8 (25^3 = 15625 | 26^3), fixed point + likes + Lmin 24 (17^3 | 18^3)
TIER_CASES = [("unit", False, 32, 33), ("real", False, 25, 26), ("real", True, 17, 18)]


@pytest.mark.parametrize("kind,likes,nb_lds,nb_glob", TIER_CASES)
def test_tier_switch_against_numpy(kind, likes, nb_lds, nb_glob):
    from getdist_amd.mcsamples import MCSamples

    N = 400_000
    r = np.random.default_rng(7)
    z = r.standard_normal((N, 3))
    z[:, 2] = np.abs(z[:, 2])
    ll = 0.5 * np.sum(z**2, axis=1)
    w = r.exponential(1.0, N) if kind == "real" else None
    mc = MCSamples(samples=z, weights=w, loglikes=ll, names=["u", "v", "t"], ranges={"t": (0, None)})
    for nb in (nb_lds, nb_glob):
        if likes:
            d = mc.getRawNDDensityGridData(["u", "v", "t"], num_bins_ND=nb, meanlikes=True, maxlikes=True)
        else:
            d = mc.getRawNDDensity(["u", "v", "t"], num_bins_ND=nb)
        H, L = _numpy_nd(mc, (0, 1, 2), nb, w, ll)
        P = _expected_P(mc, (0, 1, 2), nb, H)
        if kind == "unit":
            assert np.array_equal(d.P, P), nb
        else:
            assert np.max(np.abs(d.P - P)) <= 1e-10 * np.max(P), nb
        if likes:
            assert np.array_equal(d.maxlikes, np.exp(-np.max(-ll) - L)), nb


def test_tiers_agree_bit_for_bit(monkeypatch):
    """The same grids through the LDS tier and forced through the global tier (GDHIP_HISTND_GLOBAL): integer sums in
    both, so bit-equal, real weights included."""
    from getdist_amd.mcsamples import MCSamples

    N = 300_000
    r = np.random.default_rng(8)
    z = r.standard_normal((N, 4))
    ll = 0.5 * np.sum(z**2, axis=1)
    mc = MCSamples(samples=z, weights=r.exponential(1.0, N), loglikes=ll, names=list("abcd"))
    lists = [["a", "b", "c"], ["b", "d"], ["a", "b", "c", "d"]]
    lds = mc.getRawNDDensities(lists, meanlikes=True, maxlikes=True)
    monkeypatch.setenv("GDHIP_HISTND_GLOBAL", "1")
    glob = mc.getRawNDDensities(lists, meanlikes=True, maxlikes=True)
    for x, y in zip(lds, glob):
        for a in ("P", "likes", "maxlikes", "contours", "maxcontours"):
            assert np.array_equal(getattr(x, a), getattr(y, a)), a


def test_grid_cap_refused_before_launch():
    from getdist_amd.mcsamples import MCSamples, SettingError

    z = np.random.default_rng(9).standard_normal((5000, 6))
    mc = MCSamples(samples=z, names=["q%d" % i for i in range(6)])
    with pytest.raises(SettingError):
        mc.getRawNDDensity(["q%d" % i for i in range(6)], num_bins_ND=20)  # 20^6 = 6.4e7 > 2^25
    # the C entry refuses the same grid itself, before it touches the (one-element) output
    import ctypes as C

    from getdist_amd import _lib

    ctx = mc.ctx
    dims = np.array([6], dtype=np.int32)
    cols = np.arange(6, dtype=np.int32)
    bmin, width, out = np.zeros(6), np.ones(6), np.zeros(1)
    pd = C.POINTER(C.c_double)
    rc = ctx.lib.gd_histnd_batch(ctx.h, 1, dims.ctypes.data_as(C.POINTER(C.c_int32)), cols.ctypes.data_as(C.POINTER(C.c_int32)),
                                 bmin.ctypes.data_as(pd), width.ctypes.data_as(pd), 20, _lib.GD_HISTND_H, -1,
                                 out.ctypes.data_as(pd), None, None)
    assert rc == _lib.GD_ERR_BADARG
    assert b"GD_HISTND_MAX_BINS" in ctx.lib.gd_last_error(ctx.h)
