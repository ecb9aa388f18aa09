"""
CPU tests of the result text (getdist_amd/types.py, MCSamples.getTable / getLatex / getInlineLatex) against what the reference
gave (tests/golden/tables.json, made by tests/golden/make_golden_tables.py): number formatting byte for byte, MargeStats /
LikeStats text and every tableTex variant from the recorded numbers, the file round trips, and the entry points end to end on
the numpy context double.
"""

import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import tables_cases as tc
from fake_ctx import FakeContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return tc.load_golden()


def ours():
    from getdist_amd import types as T
    from getdist_amd.paramnames import ParamInfo

    return T, (lambda rec: tc.marge_from_numbers(T.MargeStats, lambda nm, lab: ParamInfo(nm, lab or None), T.ParamLimit, rec))


def test_format_vectors_are_byte_equal(gold):
    """NumberFormatter.namesigFigs / formatNumber on every recorded vector: random magnitudes 1e-8..1e8 with error ratios
    1e-4..10, both signs, Python floats and numpy.float64, carries, exact halves, the thresholds at 20 / 100 / 1000 and the
    fixed-point fallback."""
    T, _ = ours()
    fmts = {"default": T.NumberFormatter(), "err1": T.NumberFormatter(err_sf=1)}
    name_inputs, num_inputs = tc.format_inputs()
    want = gold["format"]
    assert len(name_inputs) == len(want["namesigFigs"]) >= 2000 and len(num_inputs) == len(want["formatNumber"]) >= 1000
    for v, w in zip(name_inputs, want["namesigFigs"]):
        assert tc.run_namesig(fmts[v["formatter"]], v) == w, v
    for v, w in zip(num_inputs, want["formatNumber"]):
        assert tc.run_format_number(fmts["default"], v) == w, v
    assert any(w.startswith("0.0|+5.0") for w in want["namesigFigs"])  # the fixed-point fallback is among them


def test_number_helpers():
    from getdist_amd import types as T

    assert T.numberFigs(9.996, 3) == "10.0" and T.numberFigs(9.996, 4) == "9.996" and T.numberFigs(99.95, 3) == "100"
    assert T.numberFigs(2.5, 1) == "3" and T.numberFigs(0.125, 2) == "0.13"  # exact halves go up
    assert T.numberFigs(0.1, 4) == "0.1000" and T.numberFigs(0.0, 3) == "0.00" and T.numberFigs(-0.00123456, 2) == "-0.0012"
    assert T.numberFigs(123456.0, 3, sci=True) == ("1.23", 5) and T.numberFigs(12345.6, 3, sci=True) == ("12300", 0)
    assert T.numberFigs(np.float32(0.5), 2) == "0.50"
    assert str(T.float_to_decimal(0.1)).startswith("0.1000000000000000055511151231257827")
    assert T.times_ten_power(-5) == "\\cdot 10^{-5}" and T.texEscapeText("a_b") == "a{\\textunderscore}b"
    nf = T.NumberFormatter()
    assert nf.decimal_places("12.345") == 3 and nf.decimal_places("12") == 0
    assert nf.plusMinusLimit(2, 1.0, -1.0) and not nf.plusMinusLimit(1, 1.0, -1.05) and nf.plusMinusLimit(1, 1.0, -1.2)
    assert [T.ParamLimit([0, 1], t).limitType() for t in ("two", ">", "<", "none")] == [
        "two tail", "one tail upper limit", "one tail lower limit", "none"]


@pytest.mark.parametrize("name", tc.ZOO_SETS + [tc.CRAFTED, tc.SYNTHETIC])
def test_recorded_numbers_give_the_recorded_text(gold, name, tmp_path):
    """MargeStats(names, limits) of the recorded numbers: str, column labels, texValues (as getLatex / getInlineLatex use it)
    and every tableTex variant byte for byte; the .margestats text read back gives the same object."""
    T, build = ours()
    g = gold["sets"][name]
    ms, part = build(g["main"]), build(g["part"])
    assert str(ms) == g["margestats"]
    assert ms.headerLine(inc_limits=True)[0] == g["header_inc_limits"]
    assert [ms.getColumnLabels(k) for k in (1, 2, 3)] == g["column_labels"]
    got = tc.all_latex(T, ms, part)
    assert sorted(got) == sorted(g["strings"])
    for key, want in g["strings"].items():
        assert got[key] == want, (name, key)
    # round trip through the file
    path = str(tmp_path / "set.margestats")
    ms.saveAsText(path)
    back = T.MargeStats().loadFromFile(path)
    assert str(back) == g["margestats"] and back.limits == g["main"]["contours"] and not back.hasBestFit
    for p, q in zip(ms.names, back.names):
        assert (q.name, q.isDerived) == (p.name, p.isDerived)
        assert [lim.limitTag() for lim in q.limits] == [lim.limitTag() for lim in p.limits]
        assert np.allclose([q.mean, q.err], [p.mean, p.err], rtol=1e-7)
        assert np.allclose([[lim.lower, lim.upper] for lim in q.limits], [[lim.lower, lim.upper] for lim in p.limits],
                           rtol=1e-7, atol=0)
    assert tc.latex_of(T, back, 2, None) == tc.latex_of(T, T.MargeStats().loadFromFile(path), 2, None)


def test_table_document_write_and_ordered_filter(gold, tmp_path):
    T, build = ours()
    g = gold["sets"][tc.CRAFTED]
    ms = build(g["main"])
    table = T.ResultTable(2, ms, limit=1)
    table.write(str(tmp_path / "t.tex"), document=True, latex_preamble=tc.PREAMBLE)
    assert (tmp_path / "t.tex").read_text(encoding="utf-8") == g["strings"]["table/document"]
    assert not hasattr(table, "tablePNG")
    # filteredCopy: deep, and in the order asked for
    sub = ms.filteredCopy(["w", "nope", "H0"])
    assert sub.list() == ["w", "H0"] and isinstance(sub, T.MargeStats) and sub.limits == ms.limits
    assert sub.names[0] is not ms.parWithName("w") and sub.names[0].limits[0] is not ms.parWithName("w").limits[0]
    assert sub.names[0].limits[0].upper == ms.parWithName("w").limits[0].upper
    rows = T.ResultTable(1, ms, limit=1, paramList=["w", "H0"]).tableTex().splitlines()
    assert [r.split("$")[1].strip() for r in rows if "boldmath" in r] == ["w_0", "H_0"]
    assert ms.parFormat() == "%-10s" and ms.maxNameLen() == 6 and ms.name(2, True) == "mass*" and ms.name(2) == "mass"
    assert ms.numParams() == 5 and T.TableFormatter().getLine("nothing of that name") == "\\hline"


def test_likestats_text_and_round_trip(gold, tmp_path):
    from getdist_amd import types as T
    from getdist_amd.paramnames import ParamInfo

    text = gold["sets"][tc.CRAFTED]["likestats"]
    path = tmp_path / "set.likestats"
    path.write_text(text, encoding="utf-8")
    ls = T.LikeStats().loadFromFile(str(path))
    assert ls.complexity is None and ls.names == []
    assert str(ls) == text.split("\n\n")[0] + "\n"  # the scalar summary; the table is not read back (as in the reference)
    table = tc.likestats_table(text)
    rec = gold["sets"][tc.CRAFTED]["main"]["params"]
    for p in rec:
        par = ParamInfo(p["name"], p["label"])
        par.isDerived = p["derived"]
        v = table[p["name"] + ("*" if p["derived"] else "")]
        par.bestfit_sample, par.ND_limit_bot, par.ND_limit_top = v[0], np.array([v[1], v[3]]), np.array([v[2], v[4]])
        ls.names.append(par)
    assert str(ls) == text and ls.headerLine() in text
    ls.saveAsText(str(path))
    assert path.read_text(encoding="utf-8") == text
    ls.names[0].ND_limit_bot = np.array([0.0])
    with pytest.raises(Exception, match="at least two contour levels"):
        str(ls)


def reference_samples(gold, factory=FakeContext, **kw):
    from getdist_amd.mcsamples import MCSamples

    inp = tc.load_inputs()
    return MCSamples(samples=inp["testTables/samples"], loglikes=inp["testTables/loglikes"], names=gold["testTables"]["names"],
                     labels=gold["testTables"]["labels"], _context_factory=factory, **kw)


def test_reference_test_tables_end_to_end(gold):
    """The two assertions of the reference's testTables (getdist_test.py:114-122) on its own sample set, through
    getMargeStats on the numpy context double; and the error paths of the entry points."""
    mc = reference_samples(gold)
    assert str(mc.getLatex(limit=2)) == "(['x', 'y'], ['0.0^{+2.1}_{-2.1}', '0.0^{+1.3}_{-1.3}'])"
    table = mc.getTable(columns=1, limit=1, paramList=["x"])
    assert r"0.0\pm 1.2" in table.tableTex()
    assert table.tableTex() == gold["testTables"]["table"] and str(mc.getLatex(limit=2)) == gold["testTables"]["latex_limit2"]
    assert mc.getInlineLatex("x") == gold["testTables"]["inline_x"] == mc.getLatex("x")
    assert mc.getLatex(["y", "nope"])[1][1] is None and mc.getLatex(["y", "nope"])[0] == ["y", None]
    assert mc.getLatex([mc.paramNames.names[1]], limit=2) == (["y"], ["0.0^{+1.3}_{-1.3}"])  # a ParamInfo, as the plotter passes
    with pytest.raises(ValueError, match="parameter nope not found"):
        mc.getInlineLatex("nope")
    with pytest.raises(NotImplementedError, match="best-fit files are outside the accelerated path"):
        mc.getTable(include_bestfit=True)
    assert tc.blank_numbers(str(mc.getMargeStats())) == tc.blank_numbers(gold["testTables"]["margestats"])
    assert tc.blank_numbers(str(mc.getLikeStats())) == tc.blank_numbers(gold["testTables"]["likestats"])
    assert not str(mc.getMargeStats()).startswith("<")


def test_entry_points_add_no_device_call_after_marge_stats(gold):
    mc = reference_samples(gold, factory=tc.counting(FakeContext))
    mc.getMargeStats()
    before = dict(mc.ctx.fetched)
    assert before["limits1d"] == 1 and before["quantiles"] >= 1
    mc.getLatex()
    mc.getInlineLatex("y", limit=2)
    mc.getTable(columns=2).tableTex()
    assert dict(mc.ctx.fetched) == before
    mc.updateSettings({"contours": [0.5, 0.9]}, doUpdate=True)  # a change of the statistics computes the limits again
    assert mc.getMargeStats().limits == [0.5, 0.9] and mc.ctx.fetched["limits1d"] == 2
    assert len(mc.paramNames.names[0].limits) == 2


def test_parameter_without_a_label_ends_its_line_as_the_reference_does(gold):
    """The zoo fixtures have no labels: the last field of their .margestats lines is empty in the reference's text, while
    getLabel() -- what tables print -- is the name."""
    from getdist_amd.mcsamples import MCSamples

    inp = tc.load_inputs()
    mc = MCSamples(samples=inp["testTables/samples"][:3000], loglikes=inp["testTables/loglikes"][:3000], names=["x", "y"],
                   _context_factory=FakeContext)
    for text in (str(mc.getMargeStats()), str(mc.getLikeStats())):
        lines = [ln for ln in text.splitlines() if ln.startswith(("x ", "y "))]
        assert len(lines) == 2 and all(ln.endswith("   ") and ln.rstrip() != ln for ln in lines), text
    assert mc.getMargeStats().parWithName("x").getLabel() == "x" and mc.getInlineLatex("x").startswith("x = ")
    assert gold["sets"]["c1_bounded"]["margestats"].splitlines()[3].endswith("   ")


DRIVER = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests")); sys.path.insert(0, %(ref)r)
    import matplotlib
    matplotlib.use("Agg")
    from getdist import plots  # before getdist_amd: its parameter objects then derive from the plotter's ParamInfo
    import tables_cases as tc
    from fake_ctx import FakeContext
    from getdist_amd.mcsamples import MCSamples
    from getdist_amd.plotting import prefill_plot_caches

    gold, inp = tc.load_golden(), tc.load_inputs()
    mc = MCSamples(samples=inp["testTables/samples"], loglikes=inp["testTables/loglikes"], names=gold["testTables"]["names"],
                   labels=gold["testTables"]["labels"], _context_factory=FakeContext)
    g = plots.get_single_plotter()
    g.sample_analyser.mcsamples["amd_chain"] = mc
    prefill_plot_caches(g.sample_analyser, "amd_chain", mc, params=["x"])
    g.plot_1d("amd_chain", "x", title_limit=1)
    print("TITLE[" + g.get_axes().get_title() + "]")
""")


def test_real_plotter_title_limit(gold):
    """Where GetDist is importable: its real plot_1d(..., title_limit=1) (plots.py:1021-1034) on a sample set of this package
    with prefilled caches asks for getInlineLatex and sets the recorded caption as the axis title."""
    ref = os.environ.get("GETDIST_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "getdist")):
        pytest.skip("GetDist is not available on this box (the caption itself is checked by test_reference_test_tables_end_to_end)")
    out = subprocess.run([sys.executable, "-c", DRIVER % dict(root=ROOT, ref=ref)], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600, env=dict(os.environ, MPLBACKEND="Agg"))
    assert out.returncode == 0, out.stdout[-3000:]
    assert "TITLE[$" + gold["testTables"]["inline_x"] + "$]" in out.stdout, out.stdout[-3000:]
