"""The inputs and calls of tests/golden/compose.npz (MCSamples.copy, getCombinedSamplesWithSamples and the look-ups and
small queries around them).  Inputs are regenerated from seeds on any box, so the golden file holds reference outputs only.
Shared by tests/golden/make_golden_compose.py and the CPU / GPU tests."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compose.npz")

SEED = 20261019  # (the streams below: 1 = A, 2 = B, 3 = MC, 4 = ONE)
FIXED_VALUE = 0.25  # the constant column c of the FX sets


def _rng(stream):
    return np.random.default_rng(np.random.SeedSequence([SEED, stream]))


def _correlated(r, rows, shift):
    """Three correlated columns with x >= 0 (so that the hard bound x >= 0 is one the samples lean on)."""
    g = r.standard_normal((rows, 3))
    mix = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [-0.3, 0.5, 0.9]])
    s = g @ mix.T * [1.0, 2.0, 0.5] + shift
    s[:, 0] = np.abs(s[:, 0])
    return s, 0.5 * np.sum(g**2, axis=1)


def fixtures():
    """name -> dict(samples, weights, loglikes, names, labels, derived, ranges)"""
    out = {}
    r = _rng(1)
    s, ll = _correlated(r, 3001, [0.0, 1.0, -2.0])
    d = s[:, 0] * s[:, 1] + 0.3 * s[:, 2]
    out["A"] = dict(samples=np.column_stack([s, d]), weights=r.gamma(2.0, 1.0, 3001), loglikes=ll + 1.5,
                    names=["x", "y", "z", "d"], labels=["x_A", "y_A", "z_A", "d_A"], derived=["d"], ranges={"x": (0, None)})
    r = _rng(2)
    s, ll = _correlated(r, 1777, [0.1, 0.8, -2.1])
    q = r.standard_normal(1777) + 0.4 * s[:, 1]
    out["B"] = dict(samples=np.column_stack([s[:, 2], s[:, 0], q, s[:, 1]]), weights=r.integers(1, 6, 1777).astype(float),
                    loglikes=ll + 0.5 * q**2, names=["z", "x", "q", "y"], labels=["z_B", "x_B", "q_B", "y_B"], derived=[],
                    ranges={"x": (0, None)})
    out["U"] = dict(out["A"], weights=None)
    out["NL"] = dict(out["B"], loglikes=None)
    a, b = out["A"], out["B"]
    out["FXA"] = dict(a, samples=np.column_stack([a["samples"], np.full(3001, FIXED_VALUE)]), names=a["names"] + ["c"],
                      labels=a["labels"] + ["c_A"])
    out["FXB"] = dict(b, samples=np.insert(b["samples"], 2, FIXED_VALUE, axis=1), names=["z", "x", "c", "q", "y"],
                      labels=["z_B", "x_B", "c_B", "q_B", "y_B"])
    r = _rng(3)
    chains, weights = [], []
    for k, rows in enumerate((700, 701, 650)):
        chains.append(_correlated(r, rows, [0.0, 1.0 + 0.05 * k, -2.0])[0])
        weights.append(r.integers(1, 4, rows).astype(float))
    out["MC"] = dict(samples=chains, weights=weights, loglikes=None, names=["x", "y", "z"], labels=None, derived=[], ranges={})
    out["ONE"] = dict(samples=_rng(4).standard_normal((17, 1)), weights=None, loglikes=None, names=["x"], labels=None,
                      derived=[], ranges={})
    return out


# combined case -> (first set, second set, sample_weights)
COMBINED = {
    "AB_11": ("A", "B", (1, 1)),
    "AB_2h": ("A", "B", (2, 0.5)),
    "AB_none": ("A", "B", None),
    "UB": ("U", "B", (1, 1)),
    "ANL": ("A", "NL", (1, 1)),
    "FX": ("FXA", "FXB", (1, 1)),
}

# the noise matrix of the signal-to-noise query: fixed, symmetric positive definite, condition number ~3
NOISE = np.array([[2.0, 0.3, -0.2], [0.3, 1.5, 0.4], [-0.2, 0.4, 1.0]])
SN_PARAMS = ["x", "y", "z"]


def build(cls, fx, settings=None, **kw):
    """The fixture as an MCSamples of class ``cls`` (the reference's or this package's; kw: e.g. _context_factory)."""
    f = fixtures()[fx]
    samples = f["samples"] if isinstance(f["samples"], list) else np.ascontiguousarray(f["samples"])
    mc = cls(samples=samples, weights=f["weights"], loglikes=f["loglikes"], names=list(f["names"]), labels=f["labels"],
             ranges=dict(f["ranges"]), settings=settings, **kw)
    for nm in f["derived"]:
        mc.paramNames.parWithName(nm).isDerived = True
    return mc


def combine(cls, case, **kw):
    first, second, sample_weights = COMBINED[case]
    return build(cls, first, **kw).getCombinedSamplesWithSamples(build(cls, second, **kw), sample_weights=sample_weights)


def limit_rows(par):
    """A parameter's marginalised limits as test_marge_stats_golden lays them out."""
    return np.array([[lim.lower, lim.upper, lim.twotail, lim.onetail_upper, lim.onetail_lower] for lim in par.limits], dtype=float)


def sign_fixed(U):
    """Eigenvector rows with the sign that makes each row's largest-magnitude entry positive."""
    U = np.array(U, dtype=float)
    for row in U:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1
    return U


def summary_numbers(text):
    """The four numbers of getNumSampleSummaryText (no indep_thin line): mean weight, total weight, sum w / max w,
    (sum w)^2 / sum w^2 -- after checking rows and parameters, which are exact."""
    lines = text.splitlines()
    assert len(lines) == 3, text
    head = lines[0].replace(",", "").replace(";", "").split()
    return ([int(head[1]), int(head[3])],
            np.array([float(head[7]), float(head[10]), float(lines[1].split(":")[-1]), float(lines[2].split(":")[-1])]))


def dict_to_arrays(d):
    """A look-up dict as (keys, values) arrays for the golden file."""
    return np.array(list(d.keys())), np.array([float(v) for v in d.values()])


def shared(gold, key):
    """An array of the golden file that several cases may share: stored once, the others hold its key under key + "@"."""
    return gold[key] if key in gold.files else gold[str(gold[key + "@"])]


def load_golden():
    return np.load(GOLDEN)
