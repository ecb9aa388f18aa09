"""
Generates tests/golden/tables.json (and tests/golden/tables_inputs.npz) by importing the REAL GetDist (the reference; build
container only): what its number formatter, its result tables and its .margestats / .likestats text give for

1. deterministic number-format vectors (NumberFormatter.namesigFigs / formatNumber),
2. the six fixtures of test_marge_stats_golden and one crafted five-parameter set (tests/tables_cases.py), each with its
   first part of rows as second / reference result,
3. the reference's own testTables (getdist/tests/getdist_test.py:114-122) on its own sample set.

The file holds strings and numbers only.  Before writing, every recorded LaTeX string is formatted again by the reference
from numbers moved by twice the gates of test_marge_stats_golden (limits +-2*(2e-5*err), mean and err +-1e-10 relative, all
sign combinations): a string that changes sits on a rounding boundary, and a device whose numbers are within the gates could
print either form.  Such a (result, parameter, limit) is named under "drop": one per set, the one nearest to its boundary,
and none of the crafted set (change its seed instead).  A set with a second one (wj1d has, at three significant figures of
the error) lists it under "near" with the multiple of the gates at which its text changes; that must be above 1, so that
numbers within the gates still give the recorded text, and the device comparison keeps it.  The maker fails otherwise.

    python tests/golden/make_golden_tables.py
"""

import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("GETDIST_REFERENCE", "/root/reference"))

from getdist import MCSamples  # noqa: E402  (the reference)
from getdist import types as T  # noqa: E402
from getdist.paramnames import ParamInfo  # noqa: E402

import tables_cases as tc  # noqa: E402
from oracle.fixtures import fixture_zoo  # noqa: E402


# ---- 1. number-format vectors ---------------------------------------------------------------------------------------------
def format_vectors():
    """The reference's results for tables_cases.format_inputs() (the inputs are regenerated there from a seed; only the
    results are stored, one "|"-joined string per vector)."""
    fmts = {"default": T.NumberFormatter(), "err1": T.NumberFormatter(err_sf=1)}
    name_inputs, num_inputs = tc.format_inputs()
    return dict(namesigFigs=[tc.run_namesig(fmts[v["formatter"]], v) for v in name_inputs],
                formatNumber=[tc.run_format_number(fmts["default"], v) for v in num_inputs])


# ---- 2. sample sets --------------------------------------------------------------------------------------------------------
def ref_stats(names, contours):
    m = T.MargeStats()
    m.hasBestFit, m.limits, m.names = False, contours, names
    return m


def ref_param(name, label):
    par = ParamInfo(name=name, label=label)
    par.label = label  # (an empty label stays empty)
    return par


def unstable_combinations(rec, build, scale):
    """The (result, parameter, limit) whose LaTeX changes when the numbers move by ``scale`` times the gates of
    test_marge_stats_golden, any combination of signs.  Checked per parameter: its getLatex forms (every err_sig_figs) and
    its shift forms against the first part for the full set, its table cell for the first part."""
    found = set()
    main0, part0 = build(rec["main"]), build(rec["part"])
    fmts = {}
    for esf in (None, 1, 3):
        fmts[esf] = T.NoLineTableFormatter()
        if esf:
            fmts[esf].numberFormatter.err_sf = esf
    shifts = list(itertools.product((False, True), (False, True)))
    for signs in itertools.product((-scale / 2, scale / 2), repeat=6):  # (a sign of 1 is twice the gates)
        main, part = build(rec["main"], signs[:4]), build(rec["part"], signs[4:] + signs[2:4])
        listed = tc.table_names(main.list())
        for limit in (1, 2, 3):
            for nm in main.list():
                if any(main.texValues(f, nm, limit) != main0.texValues(f, nm, limit) for f in fmts.values()):
                    found.add(("main", nm, limit))
        for nm in listed:  # (the shift forms are recorded at limit 1, the first part's own cells at limit 2)
            if any(main.texValues(fmts[None], nm, 1, part, i, s_) != main0.texValues(fmts[None], nm, 1, part0, i, s_)
                   for i, s_ in shifts):
                found.add(("main", nm, 1))
            if part.texValues(fmts[None], nm, 2) != part0.texValues(fmts[None], nm, 2):
                found.add(("part", nm, 2))
    return found


def sample_set_golden(zoo, name, inputs):
    main, part = tc.make_pair(MCSamples, zoo, name, inputs)
    ms, ms_part = main.getMargeStats(), part.getMargeStats()
    out = dict(main=tc.marge_numbers(ms), part=tc.marge_numbers(ms_part), margestats=str(ms))
    out["header_inc_limits"] = ms.headerLine(inc_limits=True)[0]
    out["column_labels"] = [ms.getColumnLabels(k) for k in (1, 2, 3)]
    if main.loglikes is not None:
        out["likestats"] = str(main.getLikeStats())
    strings = tc.all_latex(T, ms, ms_part)
    # the helpers of tables_cases restate getLatex / getInlineLatex / getTable: they must give what the sample set gives
    for limit, esf in tc.LATEX_CASES:
        got = main.getLatex(limit=limit, err_sig_figs=esf)
        assert [list(got[0]), list(got[1])] == strings["latex/%d/%s" % (limit, esf)], (name, limit, esf)
    for nm in ms.list():
        for limit in tc.INLINE_LIMITS:
            assert main.getInlineLatex(nm, limit=limit) == strings["inline/%s/%d" % (nm, limit)]
    for key, spec in tc.table_variants(tc.table_names(ms.list())).items():
        assert tc.render_table(T, main, part, spec, ms.list()) == strings["table/" + key], (name, key)
    out["strings"] = strings
    # ... and the recorded numbers alone must give them back (floats survive JSON by repr)
    rec = json.loads(json.dumps(out))
    build = lambda r, signs=None: tc.marge_from_numbers(ref_stats, ref_param, T.ParamLimit, r, signs)  # noqa: E731
    assert tc.all_latex(T, build(rec["main"]), build(rec["part"])) == rec["strings"], name
    # the perturbation check: whole strings at twice the gates, then the (result, parameter, limit) behind each change
    moved_strings = set()
    for signs in itertools.product((-1, 1), repeat=6):
        moved = tc.all_latex(T, build(rec["main"], signs[:4]), build(rec["part"], signs[4:] + signs[2:4]))
        moved_strings.update(key for key, want in rec["strings"].items() if moved[key] != want)
    flips = {}  # (result, parameter, limit) -> the smallest multiple of the gates at which its LaTeX changes
    if moved_strings:
        for scale in (2.0, 1.5, 1.0, 0.5, 0.25):
            for combo in unstable_combinations(rec, build, scale):
                flips[combo] = scale
    assert bool(flips) == bool(moved_strings), (name, flips, moved_strings)
    ranked = sorted(flips, key=lambda c: (flips[c], c))
    out["drop"] = [list(c) for c in ranked[:1]]
    out["near"] = [list(c) + [flips[c]] for c in ranked[1:]]
    out["moved_strings"] = sorted(moved_strings)
    return out


def synthetic_golden():
    """Hand-made numbers for the forms no sample set above reaches: two-tail constraints with a power of ten taken out
    (large, tiny, negative), an unconstrained parameter beside a reference result, and parameters that only one of the two
    results has.  Formatter tests on the CPU only: there are no samples behind them."""
    def par(name, label, mean, err, lims, derived=False):
        return dict(name=name, label=label, derived=derived, mean=mean, err=err, limits=lims)

    contours = [0.68, 0.95, 0.99]
    main = dict(contours=contours, params=[
        par("big", "A_{\\rm big}", 3.2171e5, 1.13e4, [[3.104e5, 3.331e5, "two"], [2.99e5, 3.44e5, "two"], [2.9e5, 3.6e5, "two"]]),
        par("tiny", "\\epsilon", 2.3456e-7, 4.1e-8, [[2.0e-7, 2.9e-7, "two"], [1.6e-7, 3.4e-7, "two"], [0.0, 3.9e-7, ">"]]),
        par("negbig", "", -4.5678e6, 2.2e5, [[-4.79e6, -4.33e6, "two"], [-5.1e6, -4.2e6, "two"], [-5.3e6, -4.0e6, "two"]], True),
        par("flat", "f_{\\rm flat}", 0.5, 0.29, [[0.0, 1.0, "none"], [0.0, 1.0, "none"], [0.0, 1.0, "none"]]),
        par("lowbig", "L", 7.7e5, 3.0e5, [[4.4e5, 2.0e6, "<"], [2.9e5, 2.0e6, "<"], [1.5e5, 2.0e6, "none"]]),
        par("only_main", "o_m", 1.234, 0.0456, [[1.19, 1.28, "two"], [1.14, 1.33, "two"], [1.1, 1.4, "two"]]),
    ])
    part = dict(contours=contours, params=[
        par("big", "A_{\\rm big}", 3.1902e5, 1.52e4, [[3.04e5, 3.35e5, "two"], [2.9e5, 3.5e5, "two"], [2.8e5, 3.7e5, "two"]]),
        par("tiny", "\\epsilon", 2.61e-7, 4.1e-8, [[2.2e-7, 3.0e-7, "two"], [1.8e-7, 3.5e-7, "two"], [0.0, 4.0e-7, ">"]]),
        par("negbig", "", -4.41e6, 2.9e5, [[-4.7e6, -4.1e6, "two"], [-5.0e6, -3.8e6, "two"], [-5.2e6, -3.6e6, "two"]], True),
        par("flat", "f_{\\rm flat}", 0.52, 0.28, [[0.0, 1.0, "none"], [0.0, 1.0, "none"], [0.0, 1.0, "none"]]),
        par("lowbig", "L", 8.1e5, 3.3e5, [[4.6e5, 2.0e6, "<"], [3.0e5, 2.0e6, "<"], [1.6e5, 2.0e6, "none"]]),
        par("only_part", "o_p", 9.87, 0.65, [[9.2, 10.5, "two"], [8.6, 11.2, "two"], [8.1, 11.9, "two"]]),
    ])
    build = lambda r: tc.marge_from_numbers(ref_stats, ref_param, T.ParamLimit, r)  # noqa: E731
    ms = build(main)
    strings = tc.all_latex(T, ms, build(part))
    assert "\\left(" in json.dumps(strings) and "---" in json.dumps(strings)
    return dict(main=main, part=part, strings=strings, margestats=str(ms), header_inc_limits=ms.headerLine(inc_limits=True)[0],
                column_labels=[ms.getColumnLabels(k) for k in (1, 2, 3)], drop=[], near=[], moved_strings=[])


# ---- 3. the reference's testTables -----------------------------------------------------------------------------------------
def reference_test_tables(arrays):
    from getdist.tests.test_distributions import Test2DDistributions

    samples = Test2DDistributions().bimodal[0].MCSamples(12000, logLikes=True, random_state=10)
    arrays["testTables/samples"], arrays["testTables/loglikes"] = samples.samples, samples.loglikes
    names = [p.name for p in samples.paramNames.names]
    latex = str(samples.getLatex(limit=2))
    table = samples.getTable(columns=1, limit=1, paramList=["x"]).tableTex()
    assert latex == "(['x', 'y'], ['0.0^{+2.1}_{-2.1}', '0.0^{+1.3}_{-1.3}'])" and r"0.0\pm 1.2" in table  # the test itself
    return dict(names=names, labels=[p.label for p in samples.paramNames.names], latex_limit2=latex, table=table,
                inline_x=samples.getInlineLatex("x", limit=1), margestats=str(samples.getMargeStats()),
                likestats=str(samples.getLikeStats()))


def main():
    zoo = {fx["name"]: fx for fx in fixture_zoo()}
    arrays = {}
    arrays["crafted/samples"], arrays["crafted/loglikes"] = tc.crafted_arrays()
    out = dict(format=format_vectors(), sets={}, testTables=reference_test_tables(arrays))
    print("format vectors: %d namesigFigs, %d formatNumber" % (len(out["format"]["namesigFigs"]), len(out["format"]["formatNumber"])))
    for name in tc.ZOO_SETS + [tc.CRAFTED]:
        g = sample_set_golden(zoo, name, arrays)
        out["sets"][name] = g
        print("%-18s %2d parameters, %3d strings, perturbation check: %d strings changed, drop %s, near %s"
              % (name, len(g["main"]["params"]), len(g["strings"]), len(g["moved_strings"]), g["drop"], g["near"]))
        assert not (g["drop"] and name == tc.CRAFTED), (name, g["drop"], g["moved_strings"])
        # the second result is this maker's choice (tables_cases.SECOND_FRACTION): none of its cells may need a drop
        assert all(which == "main" for which, *_ in g["drop"] + g["near"]), (name, g["drop"], g["near"])
        # a second combination of one set can only stay in the device comparison if the gates themselves pin its text
        assert all(scale > 1.0 for *_, scale in g["near"]), (name, g["near"])
    out["sets"][tc.SYNTHETIC] = synthetic_golden()
    forms = " ".join(out["sets"][tc.CRAFTED]["strings"]["latex/1/None"][1] + out["sets"][tc.CRAFTED]["strings"]["latex/2/None"][1])
    for piece in ("\\pm", "^{+", "< ", "> ", "\\cdot 10^{", "\\nu\\rm"):  # every form but "---" comes from the crafted set
        assert piece in forms, (piece, forms)
    np.savez_compressed(os.path.join(HERE, "tables_inputs.npz"), **arrays)
    with open(os.path.join(HERE, "tables.json"), "w", encoding="utf-8") as f:
        f.write(tc.compact_json(out) + "\n")
    print("wrote tables.json (%d bytes), tables_inputs.npz (%d bytes)"
          % (os.path.getsize(os.path.join(HERE, "tables.json")), os.path.getsize(os.path.join(HERE, "tables_inputs.npz"))))


if __name__ == "__main__":
    main()
