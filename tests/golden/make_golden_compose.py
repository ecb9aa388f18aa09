"""
Generates tests/golden/compose.npz: what the reference GetDist's getCombinedSamplesWithSamples, getParamSampleDict,
getParamBestFitDict, getBounds, getCorrelatedVariable2DPlots, getNumSampleSummaryText and getSignalToNoise give on the
seeded inputs of tests/compose_cases.py (build box only: it imports the reference, which never travels).  Only reference
OUTPUTS are stored; the seeds are compose_cases.SEED = 20261019 with streams 1 (A), 2 (B), 3 (MC), 4 (ONE).

    python tests/golden/make_golden_compose.py
"""

import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
if os.environ.get("GETDIST_REFERENCE"):  # a checkout of the reference GetDist (else the installed getdist)
    sys.path.insert(0, os.environ["GETDIST_REFERENCE"])

from getdist import MCSamples  # noqa: E402  (the reference)

import compose_cases as cc  # noqa: E402

logging.getLogger().setLevel(logging.ERROR)


def put_dict(out, key, d):
    out[key + "/keys"], out[key + "/values"] = cc.dict_to_arrays(d)


def put_shared(out, key, arr):
    """Store ``arr``, or the key of an equal array already stored (the combined cases share rows): compose_cases.shared."""
    for k, v in out.items():
        if isinstance(v, np.ndarray) and v.shape == arr.shape and v.dtype == arr.dtype and np.array_equal(v, arr):
            out[key + "@"] = np.array(k)
            return
    out[key] = np.array(arr)


def main():
    out = {}
    for case in cc.COMBINED:
        ref = cc.combine(MCSamples, case)
        ref.updateBaseStatistics()
        key = "comb/" + case
        out[key + "/names"] = np.array(ref.paramNames.list())
        out[key + "/labels"] = np.array(ref.paramNames.labels())
        out[key + "/derived"] = np.array([p.isDerived for p in ref.paramNames.names])
        put_shared(out, key + "/samples", ref.samples)
        put_shared(out, key + "/weights", ref.weights)
        out[key + "/has_loglikes"] = np.bool_(ref.loglikes is not None)
        if ref.loglikes is not None:
            put_shared(out, key + "/loglikes", ref.loglikes)
        out[key + "/means"] = ref.means
        out[key + "/cov"] = ref.fullcov
        d = ref.get1DDensity("x")
        out[key + "/x_P"] = d.P
        out[key + "/x_x0x1"] = np.array([d.x[0], d.x[-1]])
        par = ref.getMargeStats().parWithName("x")
        out[key + "/x_lims"] = cc.limit_rows(par)
        out[key + "/x_meanerr"] = np.array([par.mean, par.err])
        if case == "FX":
            put_dict(out, key + "/fixed", ref.ranges.fixedValueDict())

    a = cc.build(MCSamples, "A")
    a.updateBaseStatistics()
    put_dict(out, "A/sample5", a.getParamSampleDict(5))
    put_dict(out, "A/sample5_noderived", a.getParamSampleDict(5, want_derived=False))
    put_dict(out, "A/bestfit_sample", a.getParamBestFitDict(best_sample=True))
    fxa = cc.build(MCSamples, "FXA")
    put_dict(out, "FXA/sample5_fixed", fxa.getParamSampleDict(5, want_fixed=True))
    put_dict(out, "FXA/sample5_nofixed", fxa.getParamSampleDict(5, want_fixed=False))

    a.getMargeStats()  # (getBounds reads the limit flags as the range logic of every parameter leaves them)
    bounds = a.getBounds()
    out["A/bounds/names"] = np.array(bounds.names)
    put_dict(out, "A/bounds/lower", bounds.lower)
    put_dict(out, "A/bounds/upper", bounds.upper)

    corr = np.abs(a.getCorrelationMatrix())
    vals = np.sort(corr[np.triu_indices(a.n, 1)])
    assert np.all(np.diff(vals) > 0), "two |corr| values tie: change the seed"
    out["A/corr_pairs_3"] = np.array(a.getCorrelatedVariable2DPlots(3))
    out["A/corr_pairs_12_2"] = np.array(a.getCorrelatedVariable2DPlots(12, nparam=2))

    out["A/summary"] = np.array(a.getNumSampleSummaryText())
    for fx in ("B", "U"):
        ref = cc.build(MCSamples, fx)
        ref.updateBaseStatistics()
        out[fx + "/summary"] = np.array(ref.getNumSampleSummaryText())

    w, U = a.getSignalToNoise(cc.SN_PARAMS, noise=cc.NOISE)
    assert np.all(np.diff(w) > 1e-3 * np.abs(w[1:])), "signal-to-noise eigenvalues too close: change the seed"
    out["A/sn_w"], out["A/sn_U"] = w, cc.sign_fixed(U)
    out["A/sn_w_only"] = a.getSignalToNoise(cc.SN_PARAMS, noise=cc.NOISE, eigs_only=True)

    path = cc.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
