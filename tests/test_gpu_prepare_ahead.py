"""
GPU tests of gd_prepare_params (include/gdhip.h): MCSamples.prepareParams(neff=False) lets the library enqueue the index
columns of the base grid and the first N_eff lag sums behind the quantile select, and the next get2DDensities picks them
up.  Everything a caller can see -- ranges, limit flags, N_eff, bandwidths, grids, the call's per-pair table -- must be
`array_equal` to a fresh object's with GDHIP_PREPARE_AHEAD=0, and the counter (enqueued, consumed, discarded) must show
that the pieces were used where they apply and dropped where they do not.

12 columns: 66 pairs take the three-stream path of the batched call (64 and more), 15 pairs the plain one.
"""

import numpy as np
import pytest
from scipy.signal import lfilter

from getdist_amd import synth

pytestmark = pytest.mark.gpu

PAIRS66 = synth.triangle_pairs(12)


def block(N, weighted=False):
    return synth.block_recipe(12, N, weighted=weighted, stream=71)


def chain(N, rho, seed=5):
    """12 columns of an AR(1) chain with lag-one correlation ``rho`` (0: independent rows), two of them mixed; no bounds"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, 12))
    if rho:
        x = lfilter([np.sqrt(1 - rho * rho)], [1.0, -rho], x, axis=0)
    x[:, 1] += 0.6 * x[:, 0]
    x *= np.linspace(0.5, 3.0, 12)[None, :]
    return np.asfortranarray(x), None, ["p%d" % k for k in range(12)], {}


def weighted_independent(N, seed=9):
    rng = np.random.default_rng(seed)
    s, _, names, ranges = chain(N, 0.0, seed)
    s[:, 1] = rng.standard_normal(N)  # (every pair on the base grid's own route: no sheared pair, no up-scaled grid)
    return s, rng.uniform(0.2, 3.7, N), names, ranges


def mc_of(recipe):
    from getdist_amd.mcsamples import MCSamples

    s, w, names, ranges = recipe
    return MCSamples(samples=s, weights=w, names=names, ranges=ranges)


def visible(mc, out):
    names = mc.paramNames.names
    dens = list(out)
    state = np.array([[p.range_min, p.range_max, p.sigma_range, float(p.has_limits_bot), float(p.has_limits_top), float(p.has_limits),
                       np.nan if p.N_eff_kde is None else p.N_eff_kde] for p in names if getattr(p, "_ranges_done", False)])
    return dict(state=state, bandwidth=np.array([d.bandwidth for d in dens], dtype=np.float64),
                branch=[d.bandwidth_branch for d in dens], grids=[np.array(d.P) for d in dens], meta=np.array(out._meta))


def equal(a, b):
    assert np.array_equal(a["state"], b["state"], equal_nan=True)
    assert np.array_equal(a["bandwidth"], b["bandwidth"], equal_nan=True) and a["branch"] == b["branch"]
    assert np.array_equal(a["meta"], b["meta"], equal_nan=True)
    assert len(a["grids"]) == len(b["grids"])
    for k, (g, h) in enumerate(zip(a["grids"], b["grids"])):
        assert g.shape == h.shape and np.array_equal(g, h), k


def on_and_off(monkeypatch, recipe, run):
    """``run(mc)`` -> the batch's results, on a fresh object each: (ahead on, its counters), ahead off"""
    monkeypatch.setenv("GDHIP_PREPARE_AHEAD", "0")
    mc0 = mc_of(recipe)
    off = visible(mc0, run(mc0))
    assert mc0.ctx.prepare_ahead_counts() == (0, 0, 0)
    monkeypatch.setenv("GDHIP_PREPARE_AHEAD", "1")
    mc1 = mc_of(recipe)
    on = visible(mc1, run(mc1))
    return on, mc1.ctx.prepare_ahead_counts(), off


def prepared_triangle(mc, pairs=PAIRS66, params=None, **kw):
    mc.prepareParams(params, neff=False)
    return mc.get2DDensities(pairs, **kw)


@pytest.mark.parametrize("N", [30011, 4096])
def test_main_path_uses_both_pieces(monkeypatch, N):
    on, counts, off = on_and_off(monkeypatch, block(N), prepared_triangle)
    equal(on, off)
    assert counts == (2, 2, 0)  # index columns and lag sums: enqueued, consumed, none discarded


def test_index_columns_from_the_bucket_columns(monkeypatch):
    # the route the 50-column triangle takes (k_bucket_lut, k_prebin_bq, k_prebin_fix from the select's bucket columns) at 12 columns
    monkeypatch.setenv("GDHIP_BUCKET_ROUTE_MIN", "12")
    on, counts, off = on_and_off(monkeypatch, block(30011), prepared_triangle)
    equal(on, off)
    assert counts == (2, 2, 0)
    monkeypatch.setenv("GDHIP_BUCKET_LIST_CAP", "64")  # tiny lists: blocks take the redo path of k_prebin_fix
    on2, counts2, off2 = on_and_off(monkeypatch, block(4096), prepared_triangle)
    equal(on2, off2)
    assert counts2 == (2, 2, 0)


def equicorrelated(N, n=20, k=16, rho=0.885, seed=11):
    """n columns, the first k of them correlated rho with one another: their k (k - 1) / 2 pairs take ONE up-scaled grid
    (0.866 < rho < 0.9035: 384 bins), which is then the call's largest class, and the base grid's class is a side class"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, n))
    x[:, :k] = np.sqrt(rho) * rng.standard_normal((N, 1)) + np.sqrt(1 - rho) * x[:, :k]
    return np.asfortranarray(x), None, ["p%d" % j for j in range(n)], {}


def test_base_grid_binned_on_the_third_context(monkeypatch):
    """120 pairs on the 384 grid, 70 on the base grid: the base grid's class is not the main one, so its fused launch goes out
    on the context the library made for itself -- not the one the index columns were enqueued on.  It must still find the
    piece (through the columns), wait for its event and count it consumed."""
    pairs = synth.triangle_pairs(20)
    on, counts, off = on_and_off(monkeypatch, equicorrelated(30011), lambda mc: prepared_triangle(mc, pairs))
    equal(on, off)
    sizes = [g.shape[0] for g in on["grids"]]
    assert sizes.count(384) == 120 and sizes.count(256) == 70
    assert counts == (2, 2, 0)


def test_pairs_that_meet_the_columns_in_another_order(monkeypatch):
    flipped = [(b, a) for a, b in PAIRS66]  # first appearance: 1, 0, 2, 3, ... -- the lag sums were enqueued for 0, 1, 2, ...
    on, counts, off = on_and_off(monkeypatch, block(30011), lambda mc: prepared_triangle(mc, flipped))
    equal(on, off)
    assert counts == (2, 2, 0)


def test_fifteen_pairs_on_the_plain_path(monkeypatch):
    cols = list(range(6))
    on, counts, off = on_and_off(monkeypatch, block(30011),
                                 lambda mc: prepared_triangle(mc, synth.triangle_pairs(6), params=cols))
    equal(on, off)
    assert counts == (1, 1, 0)  # (too few pairs for the byte-index route: the lag sums only)


def test_real_weights_take_the_lag_sums_only(monkeypatch):
    on, counts, off = on_and_off(monkeypatch, weighted_independent(30011), prepared_triangle)
    equal(on, off)
    assert counts == (1, 1, 0)


def test_mildly_correlated_chain_lag_two_rides(monkeypatch):
    # rho = 0.5: the probe falls below 5 % at lag 5, so the chain is still correlated at lag 1 and lag 2 rides in the launch
    on, counts, off = on_and_off(monkeypatch, chain(30011, 0.5), prepared_triangle)
    equal(on, off)
    assert counts == (2, 2, 0)


@pytest.mark.parametrize("rho", [0.9, 0.97])
def test_chain_that_outlasts_the_probe(monkeypatch, rho):
    # rho^7 > 5 %: the 8-lag probe cannot bound the correlation length, no lag sums are planned ahead (the batched call
    # reports the long route and the Python side computes N_eff); the index columns are still enqueued and used
    on, counts, off = on_and_off(monkeypatch, chain(30011, rho), prepared_triangle)
    equal(on, off)
    assert counts == (1, 1, 0)


def test_subset_prepared_superset_asked(monkeypatch):
    on, counts, off = on_and_off(monkeypatch, block(30011), lambda mc: prepared_triangle(mc, params=list(range(8))))
    equal(on, off)
    assert counts == (1, 0, 1)  # lag sums of 8 columns, asked for 12: waited for and dropped


def test_fine_bins_changed_between_the_calls(monkeypatch):
    on, counts, off = on_and_off(monkeypatch, block(30011), lambda mc: prepared_triangle(mc, fine_bins_2D=128))
    equal(on, off)
    assert counts == (2, 1, 1)  # the byte-index columns of the 256 grid have no taker


def test_invalidated_index_columns_are_binned_again(monkeypatch):
    def run(mc):
        mc.prepareParams(neff=False)
        mc.ctx.batch2d_invalidate()
        return mc.get2DDensities(PAIRS66)

    on, counts, off = on_and_off(monkeypatch, block(30011), run)
    equal(on, off)
    assert counts == (2, 1, 1)


def test_samples_edited_between_the_calls(monkeypatch):
    keep = np.random.default_rng(3).random(30011) < 0.8

    def run(mc):
        mc.prepareParams(neff=False)
        mc.filter(keep)  # the edit funnel: pending pieces are dropped behind their events
        return mc.get2DDensities(PAIRS66)

    on, counts, off = on_and_off(monkeypatch, block(30011), run)
    equal(on, off)
    assert counts[0] == 2 and counts[1] == 0 and counts[2] == 2


def test_object_closed_with_pieces_pending(monkeypatch):
    monkeypatch.setenv("GDHIP_PREPARE_AHEAD", "1")
    for twin_first in (False, True):
        mc = mc_of(block(30011))
        mc.prepareParams(neff=False)
        assert mc.ctx.prepare_ahead_counts() == (2, 0, 0)
        twin = mc._twin
        assert twin is not None
        if twin_first:
            mc._drop_second_lane()
            mc.ctx.close()
        else:
            mc.ctx.close()
            twin.ctx.close()
            mc._twin = None
        assert mc.ctx.h is None
