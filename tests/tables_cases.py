"""
Cases of the result-text goldens (tests/golden/tables.json), shared by the maker (tests/golden/make_golden_tables.py, which
runs them on the reference), the CPU tests (tests/test_tables_cpu.py: this package's formatters on the recorded numbers) and
the GPU tests (tests/test_gpu_tables.py: the device's numbers).  Every function takes the ``types`` module to use, so the
same case runs on getdist.types and on getdist_amd.types.
"""

import itertools
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZOO_SETS = ["shapes", "c1_bounded", "block10_weighted", "wj1d", "wj2d", "wj2d_weighted"]  # those of test_marge_stats_golden
CRAFTED = "crafted"
SYNTHETIC = "synthetic"  # hand-made numbers without samples (formatter tests on the CPU only)
LATEX_CASES = [(limit, esf) for limit in (1, 2, 3) for esf in (None, 1, 3)]
INLINE_LIMITS = (1,)
MAX_TABLE_PARAMS = 5  # tables of the larger fixtures list their first five parameters (5 is no multiple of 2 or 3)
TITLES = ["All rows", "First_rows"]  # (the underscore goes through texEscapeText)
PREAMBLE = "\\newcommand{\\lcdm}{\\Lambda{\\rm CDM}}"


def load_golden():
    with open(os.path.join(GOLDEN_DIR, "tables.json"), encoding="utf-8") as f:
        return json.load(f)


def load_inputs():
    return np.load(os.path.join(GOLDEN_DIR, "tables_inputs.npz"))


def compact_json(obj, indent=0):
    """JSON with one line per record: dicts open one line per key, lists of records one line per record, long lists of
    short strings twelve to a line -- so that the file stays small and a change of it shows as the lines that changed."""
    pad = " " * indent
    if isinstance(obj, dict) and "mean" not in obj:
        items = ["%s %s: %s" % (pad, json.dumps(k), compact_json(obj[k], indent + 1)) for k in sorted(obj)]
        return "{\n" + ",\n".join(items) + "\n" + pad + "}"
    if isinstance(obj, list) and obj and all(isinstance(v, dict) for v in obj):
        return "[\n" + ",\n".join(pad + " " + json.dumps(v, sort_keys=True) for v in obj) + "\n" + pad + "]"
    if isinstance(obj, list) and len(obj) > 40:
        rows = [", ".join(json.dumps(v) for v in obj[k:k + 12]) for k in range(0, len(obj), 12)]
        return "[\n" + ",\n".join(pad + " " + r for r in rows) + "\n" + pad + "]"
    return json.dumps(obj, sort_keys=True)


# ---- number-format vectors -------------------------------------------------------------------------------------------------
HAND_VALUES = [9.996, 0.09996, 99.95, 2.5, 0.125, 0.1, 0.0, 19.99, 20.0, 20.01, 99.99, 100.0, 100.1, 999.9, 1000.0, 1000.4,
               0.0012, -0.0012, 67.36, 23456.7, 1.2345e-7, 9.9996e5, -9.996, 1e-5, 123456.0]


def format_inputs():
    """(namesigFigs inputs, formatNumber inputs), deterministic: magnitudes 1e-8..1e8, error / value ratios 1e-4..10, both
    signs, Python floats and numpy.float64, both formatters' error figures; then the hand-picked values (carries, exact
    halves, 0.1, 0, either side of 20 / 100 / 1000), errors of 2 and more on values of 20 and more, and values that lose
    every figure at their errors' precision (the fixed-point fallback, with and without its plain zero)."""
    rng = np.random.default_rng(20240607)
    name_vecs, num_vecs = [], []

    def add_name(value, plus, minus, want_sign, sci, as_numpy, fmt_tag="default"):
        name_vecs.append(dict(args=[float(value), float(plus), float(minus), bool(want_sign), bool(sci)], numpy=bool(as_numpy),
                              formatter=fmt_tag))

    def add_num(value, sig_figs, want_sign, sci, as_numpy):
        num_vecs.append(dict(args=[float(value), sig_figs, bool(want_sign), bool(sci)], numpy=bool(as_numpy)))

    for k in range(2000):
        value = float(10.0 ** rng.uniform(-8, 8)) * (1 if rng.random() < 0.6 else -1)
        plus = abs(value) * float(10.0 ** rng.uniform(-4, 1))
        symmetric = rng.random() < 0.3
        minus = plus if symmetric else -plus * float(rng.uniform(0.4, 1.6))
        add_name(value, plus, minus, not symmetric, bool(k % 2), bool((k // 2) % 2), "err1" if k % 7 == 0 else "default")
    for value in HAND_VALUES:
        for ratio in (0.003, 0.04, 0.3, 2.0):
            scale = abs(value) if value else 1.0
            for sci in (False, True):
                add_name(value, scale * ratio, -scale * ratio * 1.3, True, sci, False)
                add_name(value, scale * ratio, scale * ratio, False, sci, True)
    for value, err in ((0.0012, 5.0), (-0.0012, 5.0), (0.04, 3.0), (-0.06, 3.0), (0.6, 30.0), (0.0, 1.0)):
        for sci in (False, True):
            add_name(value, err, -err, True, sci, False)
    for value, err in ((25.0, 6.0), (42.0, 2.0), (42.0, 1.9), (20.0, 8.0), (99.0, 30.0), (150.0, 40.0)):
        add_name(value, err, -0.8 * err, True, False, False)
        add_name(value, err, -0.8 * err, True, True, True)
    for k in range(600):
        value = float(10.0 ** rng.uniform(-8, 8)) * (1 if rng.random() < 0.6 else -1)
        add_num(value, [None, 1, 2, 3, 4, 6][k % 6], bool((k // 6) % 2), bool((k // 12) % 2), bool((k // 24) % 2))
    for value in HAND_VALUES + [-v for v in HAND_VALUES]:
        for sf in (None, 1, 2, 3):
            for want_sign, sci in itertools.product((False, True), (False, True)):
                add_num(value, sf, want_sign, sci, False)
    return name_vecs, num_vecs


def run_namesig(formatter, v):
    value, plus, minus, want_sign, sci = v["args"]
    cast = np.float64 if v["numpy"] else float
    return "|".join(str(x) for x in formatter.namesigFigs(cast(value), cast(plus), cast(minus), wantSign=want_sign, sci=sci))


def run_format_number(formatter, v):
    value, sig_figs, want_sign, sci = v["args"]
    res = formatter.formatNumber((np.float64 if v["numpy"] else float)(value), sig_figs, want_sign, sci)
    return "|".join(str(x) for x in res) if sci else res


# ---- the crafted five-parameter set -----------------------------------------------------------------------------------
CRAFTED_SEED, CRAFTED_ROWS = 7, 3000
CRAFTED_NAMES = ["tau", "H0", "mass", "chi2_x", "w"]
CRAFTED_LABELS = ["\\tau_{\\rm reio}", "H_0", "M_{\\rm halo}", "\\chi^2_{x}", "w_0"]
CRAFTED_RANGES = {"tau": (0.0, None), "w": (None, -0.3)}
CRAFTED_DERIVED = ["mass"]


def crafted_arrays(seed=CRAFTED_SEED, rows=CRAFTED_ROWS):
    """One-sided at 0 with values near 1e-5 (exponent form), a mean above 20 with a wide error, a skewed derived parameter
    near 1e4, a chi2* name, and one piled up against an upper bound; loglikes of the Gaussian parts."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((rows, 4))
    tau = np.abs(z[:, 0]) * 1.1e-5
    h0 = 30.0 + 5.0 * z[:, 1]
    mass = 1.0e4 * np.exp(0.45 * z[:, 2])
    chi2 = rng.chisquare(3, rows)
    w = -0.3 - np.abs(z[:, 3]) * 0.4
    samples = np.column_stack([tau, h0, mass, chi2, w])
    loglikes = 0.5 * np.sum(z ** 2, axis=1) + 0.5 * chi2
    return samples, loglikes


def sample_set_inputs(zoo, name, inputs=None):
    """Constructor keywords of sample set ``name`` (both for getdist.MCSamples and getdist_amd's) and its derived names."""
    if name == CRAFTED:
        inputs = load_inputs() if inputs is None else inputs
        return dict(samples=np.array(inputs["crafted/samples"]), loglikes=np.array(inputs["crafted/loglikes"]),
                    names=list(CRAFTED_NAMES), labels=list(CRAFTED_LABELS), ranges=dict(CRAFTED_RANGES)), list(CRAFTED_DERIVED)
    fx = zoo[name]
    return dict(samples=np.ascontiguousarray(fx["samples"]), weights=fx["weights"], names=list(fx["names"]),
                ranges=fx["ranges"]), []


SECOND_FRACTION = 0.6  # (at 0.5 two cells of the second result sit on a rounding boundary: see the maker)


def first_part(kw):
    """The same set restricted to its first rows (SECOND_FRACTION of them): the second result of the comparison tables and
    the reference result of the shift-in-sigma forms."""
    part = int(len(kw["samples"]) * SECOND_FRACTION)
    out = dict(kw, samples=kw["samples"][:part].copy())
    for k in ("weights", "loglikes"):
        if kw.get(k) is not None:
            out[k] = np.asarray(kw[k])[:part].copy()
    return out


def make_pair(cls, zoo, name, inputs=None, **extra):
    """(sample set, its first part) of class ``cls`` with the derived flags set"""
    kw, derived = sample_set_inputs(zoo, name, inputs)
    out = []
    for k in (kw, first_part(kw)):
        mc = cls(**k, **extra)
        for nm in derived:
            mc.paramNames.parWithName(nm).isDerived = True
        out.append(mc)
    return out


def counting(cls):
    """``cls`` (a device context class, or its numpy double) with a counter of the public methods fetched from it: the host
    layer fetches a context method only to call it (or, with hasattr, to decide to), so an unchanged counter means no call."""
    import collections

    class Counting(cls):
        def __init__(self, *a, **k):
            object.__setattr__(self, "fetched", collections.Counter())
            super().__init__(*a, **k)

        def __getattribute__(self, name):
            value = super().__getattribute__(name)
            if not name.startswith("_") and name != "fetched" and callable(value):
                object.__getattribute__(self, "fetched")[name] += 1
            return value

    return Counting


# ---- numbers <-> MargeStats ---------------------------------------------------------------------------------------------
def marge_numbers(ms):
    """What tables.json keeps of a MargeStats: floats survive JSON exactly (repr round trip)."""
    return dict(contours=[float(c) for c in ms.limits],
                params=[dict(name=p.name, label=p.label, derived=bool(p.isDerived), mean=float(p.mean), err=float(p.err),
                             limits=[[float(lim.lower), float(lim.upper), lim.limitTag()] for lim in p.limits])
                        for p in ms.names])


def marge_from_numbers(new_stats, new_param, limit_cls, rec, signs=None):
    """A MargeStats from recorded numbers.  ``new_stats(names, contours)`` and ``new_param(name, label)`` build the two
    objects of the module under test.  ``signs`` = (mean, err, lower, upper) in {-1, 0, +1} moves every number by that many
    perturbation steps: 1e-10 relative for mean and err, 2 * (2e-5 * err) for the limits (twice the gates of
    test_marge_stats_golden)."""
    sm, se, sl, su = signs or (0, 0, 0, 0)
    names = []
    for p in rec["params"]:
        par = new_param(p["name"], p["label"])
        par.isDerived = p["derived"]
        par.mean = p["mean"] * (1 + sm * 1e-10)
        par.err = p["err"] * (1 + se * 1e-10)
        step = 2 * 2e-5 * p["err"]
        par.limits = [limit_cls([lo + sl * step, hi + su * step], tag) for lo, hi, tag in p["limits"]]
        names.append(par)
    return new_stats(names, list(rec["contours"]))


# ---- the recorded strings --------------------------------------------------------------------------------------------------
def latex_of(T, ms, limit, err_sig_figs, params=None):
    """What MCSamples.getLatex returns (mcsamples.py:2390-2422), from a MargeStats alone"""
    fmt = T.NoLineTableFormatter()
    if err_sig_figs:
        fmt.numberFormatter.err_sf = err_sig_figs
    labels, texs = [], []
    for nm in ms.list() if params is None else params:
        tex = ms.texValues(fmt, nm, limit=limit)
        texs.append(None if tex is None else tex[0])
        labels.append(None if tex is None else ms.parWithName(nm).getLabel())
    return [labels, texs]


def inline_of(T, ms, name, limit):
    labels, texs = latex_of(T, ms, limit, None, [name])
    return labels[0] + (" " if texs[0][0] in "<>" else " = ") + texs[0]


def table_variants(names):
    """{key: spec} of the tableTex variants; ``names`` are the parameters the tables of this set list."""
    v = {}
    for cols, limit in itertools.product((1, 2, 3), (1, 2)):
        v["columns%d/limit%d" % (cols, limit)] = dict(columns=cols, limit=limit)
    v["paramList"] = dict(columns=1, limit=1, paramList=names[::2])
    v["two_results"] = dict(columns=2, limit=2, two=True)
    v["blockEnd"] = dict(columns=1, limit=2, blockEnd=[names[1], names[-2]])
    for f in ("TableFormatter", "OpenTableFormatter", "NoLineTableFormatter"):
        v["formatter/" + f] = dict(columns=1, limit=2, two=True, formatter=f, blockEnd=[names[0]])
    v["formatter/TableFormatter/columns2"] = dict(columns=2, limit=1, formatter="TableFormatter")
    for indep, subset in itertools.product((False, True), (False, True)):
        v["ref/indep%d/subset%d" % (indep, subset)] = dict(columns=1, limit=1, ref=True, indep=indep, subset=subset)
    v["document"] = dict(columns=2, limit=1, document=True)
    return v


def table_names(all_names):
    return list(all_names[:MAX_TABLE_PARAMS])


def render_table(T, main, part, spec, all_names):
    """tableTex of one variant.  ``main`` / ``part``: MargeStats, or sample sets (ResultTable asks them for theirs)."""
    names = table_names(all_names)
    kw = dict(limit=spec["limit"])
    if "paramList" in spec or len(names) < len(all_names):
        kw["paramList"] = spec.get("paramList", names)
    if spec.get("formatter"):
        kw["formatter"] = getattr(T, spec["formatter"])()
    if spec.get("two"):
        kw["titles"] = TITLES
    if spec.get("blockEnd"):
        kw["blockEndParams"] = spec["blockEnd"]
    if spec.get("ref"):
        kw.update(refResults=part if not hasattr(part, "getMargeStats") else part.getMargeStats(),
                  shiftSigma_indep=spec["indep"], shiftSigma_subset=spec["subset"])
    table = T.ResultTable(spec["columns"], [main, part] if spec.get("two") else main, **kw)
    if spec.get("document"):
        return table.tableTex(document=True, latex_preamble=PREAMBLE)
    return table.tableTex()


def all_latex(T, main, part):
    """{key: LaTeX} of everything recorded per sample set that depends only on the two MargeStats"""
    out = {}
    for limit, esf in LATEX_CASES:
        out["latex/%d/%s" % (limit, esf)] = latex_of(T, main, limit, esf)
    for nm in main.list():
        for limit in INLINE_LIMITS:
            out["inline/%s/%d" % (nm, limit)] = inline_of(T, main, nm, limit)
    for key, spec in table_variants(table_names(main.list())).items():
        out["table/" + key] = render_table(T, main, part, spec, main.list())
    return out


def dropped(drops, which, limit):
    """Names of the parameters of result ``which`` ("main" / "part") whose text at ``limit`` the maker found on a rounding
    boundary (tables.json "drop": [[result, parameter, limit]]): the device comparison leaves those entries out, the CPU
    formatter tests do not."""
    return {par for w, par, lim in drops if w == which and lim == limit}


def rows_without(text, labels):
    """The lines of a table but those of the parameters labelled ``labels``"""
    return [ln for ln in text.splitlines() if not any("$%s " % lab in ln or "$%s$" % lab in ln for lab in labels)]


# ---- .margestats / .likestats text: layout and numbers apart --------------------------------------------------------------
def blank_numbers(text):
    """The text with every %15.7E field replaced by a placeholder of the same width (and the %f numbers of the likestats
    summary by one token): what is left is the layout -- header, names with *, tags, labels, column widths."""
    import re

    text = re.sub(r"[ -]\d\.\d{7}E[+-]\d{2,3}", lambda m: "#" * len(m.group(0)), text)
    return re.sub(r"= -?\d+\.\d{6}$", "= #", text, flags=re.M)


def likestats_table(text):
    """name -> the five numbers of the table under a likestats summary"""
    out = {}
    body = text.split("\n\n", 1)[1].splitlines()[1:]
    for line in body:
        items = line.split()
        out[items[0]] = [float(v) for v in items[1:6]]
    return out
