"""The inputs and calls of tests/golden/single_samples.npz (MCSamples.makeSingleSamples and
WeightedSamples.random_single_samples_indices).  Inputs are regenerated from seeds on any box, so the golden file holds
reference outputs only.  Shared by tests/golden/make_golden_single.py and the CPU / GPU tests."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "single_samples.npz")


def _rng(stream):
    return np.random.default_rng(np.random.SeedSequence([20261018, stream]))


def fixtures():
    """name -> dict(samples, weights, loglikes, names)"""
    out = {}
    r = _rng(1)
    s = r.standard_normal((3000, 3)) * [1.0, 0.2, 5.0] + [0.0, 1.0, -3.0]
    out["unit"] = dict(samples=s, weights=None, loglikes=0.5 * np.sum(r.standard_normal((3000, 3)) ** 2, axis=1))
    r = _rng(2)
    s = r.standard_normal((5000, 4))
    out["int"] = dict(samples=s, weights=r.integers(1, 12, 5000).astype(float), loglikes=0.5 * np.sum(s**2, axis=1))
    r = _rng(3)
    s = r.standard_normal((4000, 3))
    out["real"] = dict(samples=s, weights=np.exp(0.7 * s[:, 0]) * r.uniform(0.2, 1.8, 4000),
                       loglikes=0.5 * np.sum(s**2, axis=1) + 2.0)
    # the set of the end-to-end GPU test: integer multiplicities, so the device's sum of the weights is exact
    r = _rng(4)
    s = r.standard_normal((20000, 6)) * [1.0, 2.0, 0.5, 1.0, 3.0, 0.1]
    out["big_int"] = dict(samples=s, weights=r.integers(1, 30, 20000).astype(float), loglikes=0.5 * np.sum(s**2, axis=1))
    for f in out.values():
        f["names"] = ["p%d" % i for i in range(f["samples"].shape[1])]
    return out


def _philox(seed):
    return np.random.Generator(np.random.Philox(seed))


# name -> (method, kwargs without random_state, random_state factory); "file" stands for a filename the caller supplies
CALLS = {
    "ix_default": ("random_single_samples_indices", {}, lambda: 3),
    "ix_thin": ("random_single_samples_indices", dict(thin=3.5), lambda: 4),
    "ix_max": ("random_single_samples_indices", dict(max_samples=500), lambda: 5),
    "ix_philox": ("random_single_samples_indices", dict(max_samples=800), lambda: _philox(9)),
    "arr_default": ("makeSingleSamples", {}, lambda: 6),
    "arr_thin": ("makeSingleSamples", dict(single_thin=2.5), lambda: np.random.default_rng(7)),
    "file_default": ("makeSingleSamples", dict(filename="file"), lambda: 8),
    "file_thin": ("makeSingleSamples", dict(filename="file", single_thin=4.0), lambda: 10),
}


# the calls made on each fixture, and its max_scatter_points setting (None: the default, 2000)
CALLS_FOR = {"unit": list(CALLS), "int": list(CALLS), "real": list(CALLS), "big_int": ["ix_max", "ix_philox", "arr_default"]}
SCATTER_POINTS = {"unit": 600, "int": 450, "real": 300, "big_int": None}


def all_cases():
    for fx, calls in CALLS_FOR.items():
        for call in calls:
            yield fx, call


def build(cls, fx, **kw):
    """The fixture as an MCSamples of class ``cls`` (the reference's or this package's; kw: e.g. _context_factory)."""
    f = fixtures()[fx]
    if SCATTER_POINTS[fx] is not None:
        kw["settings"] = dict(max_scatter_points=SCATTER_POINTS[fx])
    return cls(samples=np.ascontiguousarray(f["samples"]), weights=f["weights"], loglikes=f["loglikes"], names=f["names"],
               **kw)


def run(mc, call, tmpdir):
    """Result of CALLS[call] on ``mc``: an int64 index array, a (K, n) array, or the text of the file written."""
    method, kw, state = CALLS[call]
    kw = dict(kw)
    if kw.get("filename") == "file":
        kw["filename"] = os.path.join(str(tmpdir), "single_%s.txt" % call)
        assert getattr(mc, method)(random_state=state(), **kw) is None
        with open(kw["filename"], encoding="utf-8") as f:
            return f.read()
    return getattr(mc, method)(random_state=state(), **kw)


def load_golden():
    return np.load(GOLDEN)
