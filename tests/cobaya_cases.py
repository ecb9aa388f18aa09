"""
Cases of the Cobaya-run goldens (tests/golden/cobaya.json), shared by the maker (tests/golden/make_golden_cobaya.py, which
runs them on the reference), the CPU tests (tests/test_cobaya_cpu.py) and the GPU tests (tests/test_gpu_cobaya.py).

A run on disk is a yaml (committed under tests/golden/cobaya/, hand-written in the format Cobaya writes: settings only) and
chain files ``root.1.txt, root.2.txt, ...`` whose numbers are generated here from a seed: ``build_run`` puts both into a
folder and returns the root.  Every function that inspects a loaded sample set or calls the interface functions takes the
object / module to use, so the same case runs on the reference and on this package.
"""

import json
import os
import shutil

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_DIR = os.path.join(GOLDEN_DIR, "cobaya")
SYNTHETIC_A = ["minuslogprior", "minuslogprior__0", "minuslogprior__ab_prior", "chi2", "chi2__gauss_like"]
SYNTHETIC_RING = ["minuslogprior", "minuslogprior__0", "chi2", "chi2__ring"]
WIDE_SAMPLED, WIDE_DERIVED = 42, 12

# name -> yaml file, data kind, number of chain files, rows per file, weights, the ignore_rows the goldens are recorded at
# (``numbers``: the run whose chain numbers this one shares)
RUNS = {
    "runA": dict(yaml="runA.updated.yaml", kind="A", files=2, rows=200, weights="int", ignore_rows=0.3,
                 columns=["a", "b", "th", "c", "d"] + SYNTHETIC_A),
    # `polychord: null` -- the reference cannot read a sampler without options (cobaya_interface.py:254 calls .get on None),
    # so runB has no load golden; runB2 is the same run with the options Cobaya itself writes out
    "runB": dict(yaml="runB.updated.yaml", kind="ring", files=1, rows=150, weights="float", ignore_rows=0,
                 columns=["x", "y", "r"] + SYNTHETIC_RING, reference_loads=False, numbers="runB2"),
    "runB2": dict(yaml="runB2.updated.yaml", kind="ring", files=1, rows=150, weights="float", ignore_rows=0,
                  columns=["x", "y", "r"] + SYNTHETIC_RING),
    "runC": dict(yaml="runC.updated.yaml", kind="post", files=2, rows=120, weights="int", ignore_rows=0.2,
                 columns=["x", "y", "z", "e", "minuslogprior", "minuslogprior__0", "chi2", "chi2__like_a"]),
    "runD": dict(yaml="runD__full.yaml", kind="ring", files=2, rows=90, weights="int", ignore_rows=0,
                 columns=["x", "y", "r"] + SYNTHETIC_RING),
    "wide": dict(yaml="wide.updated.yaml", kind="wide", files=2, rows=64, weights="int", ignore_rows=0,
                 columns=["sampled_parameter_%02d" % i for i in range(WIDE_SAMPLED)]
                 + ["derived_parameter_%02d" % i for i in range(WIDE_DERIVED)]
                 + ["minuslogprior", "minuslogprior__0", "chi2", "chi2__wide_like"]),
}
LOADED_RUNS = [name for name, run in RUNS.items() if run.get("reference_loads", True)]
SAMPLE_ROW = 3
UNKNOWN_NAME = "no_such_parameter"


def load_golden():
    with open(os.path.join(GOLDEN_DIR, "cobaya.json"), encoding="utf-8") as f:
        return json.load(f)


# ---- chain numbers ---------------------------------------------------------------------------------------------------------
def chain_columns(name, k):
    """The (rows, 2 + parameters) array of chain file ``k`` (1-based) of run ``name``: weight, minus log posterior, then the
    run's columns.  Prior columns that a flat prior leaves constant are constant here too (the load turns them into fixed
    ranges)."""
    run = RUNS[name]
    n = run["rows"]
    rng = np.random.default_rng([20241020, sorted(RUNS).index(run.get("numbers", name)), k])
    weight = rng.integers(1, 5, n).astype(float) if run["weights"] == "int" else rng.random(n) ** 3 + 1e-3
    z = rng.standard_normal((n, 4))
    chi2 = rng.chisquare(3, n)
    if run["kind"] == "A":
        a = np.clip(3.0 - 0.8 * np.abs(z[:, 0]), 0.0, 3.0)  # piled up against the hard upper bound
        b = 1.0 + 2.0 * z[:, 1]
        th = rng.random(n) * 2 * np.pi                      # flat over the period
        pars = [a, b, th, a * b, a ** 2, np.full(n, 1.5), np.full(n, 1.0), np.full(n, 0.5), chi2, chi2]
        prior = 1.5
    elif run["kind"] in ("ring", "post"):
        x = np.clip(1.5 * z[:, 0], -5, 5)
        y = rng.random(n)
        flat = np.full(n, np.log(10.0))
        pars = [x, y, np.hypot(x, y)] if run["kind"] == "ring" else [x, y, x * y, x + y]
        pars += [flat, flat, chi2, chi2]
        prior = np.log(10.0)
    else:
        p = rng.standard_normal((n, WIDE_SAMPLED)) * 10.0 ** rng.uniform(-3, 3, WIDE_SAMPLED)
        d = np.cumsum(p, axis=1)[:, :WIDE_DERIVED]
        prior = 0.5 * z[:, 0] ** 2
        pars = list(p.T) + list(d.T) + [prior, prior, chi2, chi2]
    out = np.column_stack([weight, prior + chi2 / 2] + pars)
    assert out.shape == (n, 2 + len(run["columns"]))
    return out


def chain_text(name, k):
    """Chain file ``k`` as Cobaya writes it: a ``#`` header line naming the columns, then ``%14.8g`` fields"""
    cols = ["weight", "minuslogpost"] + RUNS[name]["columns"]
    width = max(14, max(len(c) for c in cols))
    head = "#" + " ".join("%*s" % (width - (i == 0), c) for i, c in enumerate(cols))
    body = [" ".join("%*s" % (width, "%.8g" % v) for v in row) for row in chain_columns(name, k).tolist()]
    return ("\n".join([head] + body) + "\n").encode("ascii")


def build_run(name, folder, root_name=None, with_yaml=True):
    """Write run ``name`` into ``folder`` (its yaml under the name Cobaya would give it, and its chain files); returns the
    root to load."""
    run = RUNS[name]
    root_name = root_name or name
    os.makedirs(folder, exist_ok=True)
    root = os.path.join(str(folder), root_name)
    if with_yaml:
        tail = run["yaml"][len(name):]  # ".updated.yaml" or "__full.yaml"
        shutil.copyfile(os.path.join(FIXTURE_DIR, run["yaml"]), root + tail)
    for k in range(1, run["files"] + 1):
        with open("%s.%d.txt" % (root, k), "wb") as f:
            f.write(chain_text(name, k))
    return root


def yaml_path(name):
    return os.path.join(FIXTURE_DIR, RUNS[name]["yaml"])


# ---- what is recorded of a loaded sample set ----------------------------------------------------------------------------------
def plain(x):
    """``x`` as JSON holds it: tuples as lists, numpy scalars as Python ones, anything else that JSON has no form for as its
    type's name (a function loaded from a yaml)"""
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return [plain(v) for v in x.tolist()]
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    if x is None or isinstance(x, str):
        return x
    return "<%s>" % type(x).__name__


def summarize(mc):
    """Everything cobaya.json records of a sample set loaded from a run (numbers apart from strings and lists: the tests
    compare the former to a tolerance)"""
    props = getattr(mc.properties, "params", mc.properties) or {}
    names = mc.paramNames.list()
    asked = names + [nm for nm in mc.ranges.names if nm not in names] + [UNKNOWN_NAME]
    row = mc.getParamSampleDict(SAMPLE_ROW)
    exact = dict(
        names=names, labels=[p.label for p in mc.paramNames.names], derived=[bool(p.isDerived) for p in mc.paramNames.names],
        renames={k: sorted(v) for k, v in mc.getRenames().items()}, ranges=str(mc.ranges), periodic=sorted(mc.ranges.periodic),
        sampler=mc.sampler, label=mc.label, temperature=props.get("temperature"), properties=plain(dict(props)),
        numrows=int(mc.numrows), chain_offsets=[int(v) for v in mc.chain_offsets], sample_row_keys=list(row),
        upper={nm: mc.getUpper(nm) for nm in asked}, lower={nm: mc.getLower(nm) for nm in asked},
        ranges_upper={nm: mc.ranges.getUpper(nm) for nm in asked}, ranges_lower={nm: mc.ranges.getLower(nm) for nm in asked})
    numbers = dict(sample_row=[float(row[k]) for k in row], means=[float(v) for v in mc.getMeans()])
    return plain(exact), numbers


# ---- the interface functions ---------------------------------------------------------------------------------------------------
def guarded(call):
    """The call's result as JSON holds it, or {"error": <exception class name>}"""
    try:
        return plain(call())
    except Exception as e:  # noqa: BLE001 -- the class is what is recorded
        return {"error": type(e).__name__}


def interface_results(ci, name, folder):
    """The results of the module ``ci``'s functions on run ``name``'s yaml: as a file name and (get_info_params) as the
    dictionary it holds.  Dictionaries are recorded as [key, value] lists: their order is part of the result."""
    root = build_run(name, folder)
    file = ci.cobaya_params_file(root)
    out = dict(params_file=os.path.basename(file) if file else None)
    entries = ci.get_info_params(file)
    out["info_params"] = [[k, plain(v)] for k, v in entries.items()]
    out["info_params_from_dict"] = list(ci.get_info_params(ci.yaml_file_or_dict(file)))
    for fn in ("get_sampler_key", "get_sampler_type", "get_sampler_temperature", "get_sample_label", "get_burn_removed"):
        out[fn] = guarded(lambda: getattr(ci, fn)(file))
    out["per_param"] = [[k, guarded(lambda: [[a, b] for a, b in ci.expand_info_param(v).items()]),
                         guarded(lambda: ci.is_sampled_param(v)), guarded(lambda: ci.is_derived_param(v)),
                         guarded(lambda: ci.get_range(v))] for k, v in entries.items()]
    return out


# single-parameter entries for get_range: every branch and every error
RANGE_CASES = [
    {"prior": [0, 1]},
    {"prior": [-2.5, None]},
    {"prior": {"min": 0.5}},
    {"prior": {"max": 4, "min": None}},
    {"prior": {"min": -1, "max": 1}, "periodic": True},
    {"prior": {"min": 0, "max": 6.28, "periodic": True}},
    {"prior": {"dist": "norm", "loc": 0, "scale": 1}},
    {"prior": {"loc": 2, "scale": 3}},
    {"prior": {"dist": "halfnorm", "loc": 1.5, "scale": 2}},
    {"prior": {"dist": "beta", "a": 2, "b": 3, "loc": -1, "scale": 4}},
    {"prior": {"dist": "expon", "scale": 2.0}},
    0.06,
    {"value": 3},
    {"value": "lambda a: 2*a", "min": 0, "max": 10},
    {"derived": True, "min": 0},
    {"derived": True, "periodic": True, "min": 0, "max": 1},
    {"latex": "x"},
    None,
    {"prior": "flat"},
    {"prior": 3.0},
    {"prior": [0, 1, 2]},
]


def range_results(ci):
    import copy

    return [guarded(lambda: ci.get_range(copy.deepcopy(case))) for case in RANGE_CASES]


def compact_json(obj, indent=0):
    """JSON with one line per key of the outer dictionaries and per record of a long list"""
    pad = " " * indent
    if isinstance(obj, dict) and indent < 3:
        items = ["%s %s: %s" % (pad, json.dumps(k), compact_json(obj[k], indent + 1)) for k in sorted(obj)]
        return "{\n" + ",\n".join(items) + "\n" + pad + "}"
    if isinstance(obj, list) and obj and all(isinstance(v, list) for v in obj) and len(json.dumps(obj)) > 120:
        return "[\n" + ",\n".join(pad + " " + json.dumps(v, sort_keys=True) for v in obj) + "\n" + pad + "]"
    return json.dumps(obj, sort_keys=True)


# ---- a stand-in for Cobaya's SampleCollection --------------------------------------------------------------------------------
class Collection:
    """What MCSamplesFromCobaya asks of a collection: ``.data`` (a DataFrame) and indexing by column name(s)"""

    def __init__(self, data):
        self.data = data

    def __getitem__(self, key):
        return self.data[key]


def collections_of(name, root):
    import pandas as pd

    cols = ["weight", "minuslogpost"] + RUNS[name]["columns"]
    return [Collection(pd.DataFrame(np.loadtxt("%s.%d.txt" % (root, k), ndmin=2), columns=cols))
            for k in range(1, RUNS[name]["files"] + 1)]
