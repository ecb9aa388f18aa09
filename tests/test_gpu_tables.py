"""
-m gpu: the result text from the real device path (MCSamples -> C ABI -> HIP kernels -> getdist_amd/types.py) against what the
reference printed (tests/golden/tables.json): getLatex / getInlineLatex / tableTex exactly -- the maker checked that numbers
within the gates of test_marge_stats_golden cannot change them, and names the entries where they could -- and the
.margestats / .likestats text by layout and, parsed back, by number at those gates.
"""

import numpy as np
import pytest

import tables_cases as tc

pytestmark = pytest.mark.gpu

SETS = tc.ZOO_SETS + [tc.CRAFTED]


@pytest.fixture(scope="module")
def gold():
    return tc.load_golden()


@pytest.fixture(scope="module")
def built(zoo):
    """name -> (sample set, its first part), each with its marginalised statistics computed once for the whole module"""
    from getdist_amd.mcsamples import MCSamples

    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tc.make_pair(MCSamples, zoo, name)
            for mc in cache[name]:
                mc.getMargeStats()
        return cache[name]

    return get


@pytest.mark.parametrize("name", SETS)
def test_latex_and_tables_from_the_device(built, gold, name):
    from getdist_amd import types as T

    main, part = built(name)
    g = gold["sets"][name]
    want = g["strings"]
    names = main.paramNames.list()
    label = {p["name"]: p["label"] or p["name"] for p in g["main"]["params"]}
    assert len(g["drop"]) <= (0 if name == tc.CRAFTED else 1)
    for limit, esf in tc.LATEX_CASES:
        labels, texs = main.getLatex(limit=limit, err_sig_figs=esf)
        skip = tc.dropped(g["drop"], "main", limit)
        want_labels, want_texs = want["latex/%d/%s" % (limit, esf)]
        assert labels == want_labels
        for nm, got_tex, want_tex in zip(names, texs, want_texs):
            assert got_tex == want_tex or nm in skip, (name, nm, limit, esf)
    for nm in names:
        for limit in tc.INLINE_LIMITS:
            if nm not in tc.dropped(g["drop"], "main", limit):
                assert main.getInlineLatex(nm, limit=limit) == want["inline/%s/%d" % (nm, limit)], (name, nm, limit)
    assert main.getLatex(names[0]) == want["inline/%s/1" % names[0]] or names[0] in tc.dropped(g["drop"], "main", 1)
    for key, spec in tc.table_variants(tc.table_names(names)).items():
        got = tc.render_table(T, main, part, spec, names)
        skip = {label[nm] for nm in tc.dropped(g["drop"], "main", spec["limit"])}
        if spec.get("two"):
            skip |= {label[nm] for nm in tc.dropped(g["drop"], "part", spec["limit"])}
        assert tc.rows_without(got, skip) == tc.rows_without(want["table/" + key], skip), (name, key)
    # the public entry point builds the same table as the constructor
    assert main.getTable(columns=2, limit=1, paramList=tc.table_names(names)).tableTex() == T.ResultTable(
        2, main.getMargeStats(), limit=1, paramList=tc.table_names(names)).tableTex()


@pytest.mark.parametrize("name", SETS)
def test_margestats_text_from_the_device(built, gold, name, tmp_path):
    """str(getMargeStats()): the layout of the reference's text, its numbers within the gates of test_marge_stats_golden."""
    from getdist_amd import types as T

    main, _ = built(name)
    g = gold["sets"][name]
    text = str(main.getMargeStats())
    assert tc.blank_numbers(text) == tc.blank_numbers(g["margestats"])
    got_path, want_path = tmp_path / "got.margestats", tmp_path / "want.margestats"
    main.getMargeStats().saveAsText(str(got_path))
    want_path.write_text(g["margestats"], encoding="utf-8")
    assert got_path.read_text(encoding="utf-8") == text
    got, ref = T.MargeStats().loadFromFile(str(got_path)), T.MargeStats().loadFromFile(str(want_path))
    assert got.limits == ref.limits == g["main"]["contours"] and got.list() == ref.list()
    for p, q, rec in zip(got.names, ref.names, g["main"]["params"]):
        assert (p.name, p.isDerived, p.label) == (q.name, q.isDerived, q.label)
        assert [lim.limitTag() for lim in p.limits] == [lim.limitTag() for lim in q.limits], (name, p.name)
        assert np.allclose([p.mean, p.err], [q.mean, q.err], rtol=1e-11, atol=0), (name, p.name)
        for a, b in zip(p.limits, q.limits):
            assert max(abs(a.lower - b.lower), abs(a.upper - b.upper)) < 2e-5 * max(1e-300, rec["err"]), (name, p.name)
        # and the text is that of the numbers the object holds
        live = main.getMargeStats().parWithName(p.name)
        assert p.mean == float("%15.7E" % live.mean) and p.limits[0].upper == float("%15.7E" % live.limits[0].upper)


def test_likestats_text_from_the_device(built, gold, tmp_path):
    """str(getLikeStats()) of the crafted set: layout, the summary at the tolerance golden_util.mutator_checks uses for
    getLikeStats (1e-9 relative), best-fit sample and N-D limits (sample values) as printed."""
    from getdist_amd import types as T

    main, _ = built(tc.CRAFTED)
    want = gold["sets"][tc.CRAFTED]["likestats"]
    text = str(main.getLikeStats())
    assert tc.blank_numbers(text) == tc.blank_numbers(want)
    paths = []
    for tag, t in (("got", text), ("want", want)):
        paths.append(tmp_path / (tag + ".likestats"))
        paths[-1].write_text(t, encoding="utf-8")
    got, ref = (T.LikeStats().loadFromFile(str(p)) for p in paths)
    for att in ("logLike_sample", "logMeanInvLike", "meanLogLike", "logMeanLike", "varLogLike"):
        assert np.isclose(getattr(got, att), getattr(ref, att), rtol=1e-9, atol=0), att
    assert tc.likestats_table(text) == tc.likestats_table(want)


def test_get_latex_after_marge_stats_issues_no_device_call(zoo):
    from getdist_amd._lib import Context
    from getdist_amd.mcsamples import MCSamples

    main, _ = tc.make_pair(MCSamples, zoo, tc.CRAFTED, _context_factory=tc.counting(Context))
    main.getMargeStats()
    before = dict(main.ctx.fetched)
    assert before["density1d_batch"] >= 1 and before["limits1d"] == 1
    labels, texs = main.getLatex()
    assert len(texs) == 5 and main.getInlineLatex("tau").startswith("\\tau_{\\rm reio} < ")
    main.getTable(columns=3).tableTex()
    assert dict(main.ctx.fetched) == before  # no batched density call, nor any other
