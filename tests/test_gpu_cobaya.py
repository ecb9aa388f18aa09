"""
-m gpu: Cobaya runs through the device path.  Loading a run adds no kernel -- its O(N) part is the chain text, which goes
through Context.parse_text (gd_parse_scan / gd_parse_rows) like any chain file -- so these tests show that files in Cobaya's
format (a ``#`` header line, ``%14.8g`` fields, ``root.N.txt``) take that route and come out bit-equal to np.loadtxt, and
that what the yaml says (hard bounds, the periodic flag, the sampler) reaches the kernels that depend on it.
"""

import os

import numpy as np
import pytest

import cobaya_cases as cc

pytestmark = pytest.mark.gpu

MEANS_RTOL = 1e-12  # the gate for host-visible statistics


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


@pytest.fixture(scope="module")
def spying_context():
    """The device context class with a record of what parse_text was asked and what it answered (the answer's array is the
    block loadNumpyTxt patches the undecided tokens into, so after the load it holds the file's values)"""
    from getdist_amd._lib import Context

    class Spy(Context):
        parsed = []

        def parse_text(self, source, **kw):
            res = super().parse_text(source, **kw)
            Spy.parsed.append((source, res))
            return res

    return Spy


@pytest.fixture(scope="module")
def run_a(tmp_path_factory, spying_context):
    """Run A loaded once from its files on the device (burn-in 0.3, no cache): (sample set, root)"""
    from getdist_amd.mcsamples import MCSamples

    root = cc.build_run("runA", tmp_path_factory.mktemp("cobaya_a"))
    del spying_context.parsed[:]
    mc = MCSamples(root=root, ignore_rows=cc.RUNS["runA"]["ignore_rows"], _no_cache=True, _context_factory=spying_context)
    return mc, root


def test_run_a_takes_the_device_route(run_a, spying_context, gold):
    mc, root = run_a
    files = ["%s.%d.txt" % (root, k) for k in (1, 2)]
    assert [src for src, _ in spying_context.parsed] == files
    for fname, (_, res) in zip(files, spying_context.parsed):
        assert res is not None, "the device declined " + os.path.basename(fname)
        want = np.loadtxt(fname, ndmin=2)  # (skips the header line itself)
        assert want.shape == (200, 12) and same_bits(res["array"], want)
    exact, numbers = cc.summarize(mc)
    want = gold["runs"]["runA"]
    for key in want["exact"]:
        assert exact[key] == want["exact"][key], key
    assert exact["names"] == ["a", "b", "th", "c", "d", "chi2", "chi2__gauss_like"] and exact["chain_offsets"] == [0, 140, 280]
    for key in want["numbers"]:
        assert np.allclose(numbers[key], want["numbers"][key], rtol=MEANS_RTOL, atol=0), key
    stacked = np.vstack([np.loadtxt(f, ndmin=2)[60:] for f in files])
    keep = [0, 1, 2, 3, 4, 8, 9]  # the columns that move
    assert same_bits(mc.samples, stacked[:, 2:][:, keep]) and same_bits(mc.weights, stacked[:, 0])


def test_wide_header_across_small_chunks(tmp_path):
    """60 columns: the header line is longer than 1200 bytes.  In 256-byte chunks the leading comment spans five of them and
    the first data line starts in the middle of one."""
    from getdist_amd import chainfiles
    from getdist_amd._lib import Context

    root = cc.build_run("wide", tmp_path)
    ctx = Context(0)
    try:
        for k in (1, 2):
            fname = "%s.%d.txt" % (root, k)
            with open(fname, "rb") as f:
                header = f.readline()
            assert header.startswith(b"#") and len(header) > 3 * 256 and len(header) % 256 not in (0, 255)
            want = np.loadtxt(fname, ndmin=2)
            assert want.shape == (64, 60)
            res = ctx.parse_text(fname, chunk_bytes=256)
            assert res is not None, "the device declined the file"
            assert same_bits(chainfiles.loadNumpyTxt(fname, ctx=ctx, _parse_args=dict(chunk_bytes=256)), want)
            assert same_bits(chainfiles.loadNumpyTxt(fname, ctx=ctx), want)  # one chunk
    finally:
        ctx.close()


def test_bounds_and_period_of_the_yaml_reach_the_densities(run_a, gold):
    """The same rows built from arrays with the recorded ranges give the same grids bit for bit: ``a`` is piled up against its
    upper bound (boundary correction), ``th`` is periodic (circular convolution)."""
    from getdist_amd.mcsamples import MCSamples

    mc, root = run_a
    g = gold["runs"]["runA"]["exact"]
    ranges = {nm: (g["ranges_lower"][nm], g["ranges_upper"][nm], nm in g["periodic"]) for nm in g["ranges_lower"]
              if g["ranges_lower"][nm] is not None or g["ranges_upper"][nm] is not None}
    assert ranges["a"] == (0.0, 3.0, False) and ranges["th"][2] and ranges["fixedp"] == (0.06, 0.06, False)
    chains = [np.loadtxt("%s.%d.txt" % (root, k), ndmin=2) for k in (1, 2)]
    direct = MCSamples(samples=[c[:, 2:] for c in chains], weights=[c[:, 0] for c in chains], loglikes=[c[:, 1] for c in chains],
                       names=cc.RUNS["runA"]["columns"], ranges=ranges, ignore_rows=cc.RUNS["runA"]["ignore_rows"])
    assert direct.paramNames.list() == mc.paramNames.list()
    assert sorted(str(direct.ranges).splitlines()) == sorted(str(mc.ranges).splitlines())  # (the dictionary is in another order)
    par = mc.paramNames.parWithName("a")
    assert par.has_limits_top and par.limmax == 3.0 and mc.paramNames.parWithName("th").periodic
    d1, want1 = mc.get1DDensity("a"), direct.get1DDensity("a")
    assert same_bits(d1.x, want1.x) and same_bits(d1.P, want1.P)
    d2, want2 = mc.get2DDensity("a", "th"), direct.get2DDensity("a", "th")
    assert same_bits(d2.x, want2.x) and same_bits(d2.y, want2.y) and same_bits(d2.P, want2.P)
    assert d1.P[-1] > 0.8 * d1.P.max()  # (the bound matters here: the density ends high at a = 3)


def test_run_b_is_uncorrelated_to_the_bandwidth(tmp_path, gold):
    """``polychord`` in the yaml -> sampler "nested" -> uncorrelated_sampler in the 1D batch settings: N_eff is
    sum(w)^2 / sum(w^2) (chains.py:689) and the bandwidth is that of the same samples built with sampler="nested"."""
    from getdist_amd.mcsamples import MCSamples

    root = cc.build_run("runB", tmp_path)
    mc = MCSamples(root=root, _no_cache=True)
    assert mc.sampler == "nested" and mc.numrows == 150
    exact = cc.summarize(mc)[0]
    assert exact == gold["runs"]["runB2"]["exact"]
    chain = np.loadtxt(root + ".1.txt", ndmin=2)
    kw = dict(samples=chain[:, 2:], weights=chain[:, 0], loglikes=chain[:, 1], names=cc.RUNS["runB"]["columns"],
              ranges={"x": (-5, 5), "y": (0, 1), "r": (0, None)})
    nested = MCSamples(sampler="nested", **kw)
    got = mc.get1DDensity("x")
    want = nested.get1DDensity("x")
    par, par_nested = mc.paramNames.parWithName("x"), nested.paramNames.parWithName("x")
    w = chain[:, 0]
    assert np.isclose(par.N_eff_kde, w.sum() ** 2 / (w ** 2).sum(), rtol=1e-12, atol=0)
    assert par.N_eff_kde == par_nested.N_eff_kde and par.kde_h == par_nested.kde_h and same_bits(got.P, want.P)
