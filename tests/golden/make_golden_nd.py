"""
Generates tests/golden/raw_nd.npz: raw N-D densities (getRawNDDensity / getRawNDDensityGridData) of the REAL GetDist from
/root/reference (build container only; the reference never travels).  Inputs are regenerated on any box from seeds by
tests/nd_cases.py (oracle/fixtures.py + getdist_amd/synth.py), so only reference OUTPUTS are stored here.

    python tests/golden/make_golden_nd.py
"""

import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")

from getdist import MCSamples  # noqa: E402  (the reference)

import nd_cases  # noqa: E402

logging.getLogger().setLevel(logging.ERROR)


def main():
    out = {}
    for fx, (s, w, names, ranges, ll, _) in nd_cases.fixtures().items():
        ref = MCSamples(samples=np.ascontiguousarray(s), weights=w, loglikes=ll, names=names, ranges=ranges)
        for i, (pars, kw, normalized) in enumerate(nd_cases.CASES[fx]):
            key = nd_cases.case_key(fx, i)
            out[key + "/spec"] = np.array(nd_cases.case_spec(fx, i))
            if normalized:
                d = ref.getRawNDDensity(pars, normalized=True, **kw)
            else:
                d = ref.getRawNDDensityGridData(pars, meanlikes=True, maxlikes=True, **kw)
                out[key + "/contours"] = np.asarray(d.contours)
                out[key + "/likes"] = d.likes
                out[key + "/maxlikes"] = d.maxlikes
                out[key + "/maxcontours"] = np.asarray(d.maxcontours)
            out[key + "/P"] = d.P
            for a, x in enumerate(d.xs):
                out[key + "/x%d" % a] = x
            out[key + "/view_ranges"] = np.array(d.view_ranges, dtype=float)
            out[key + "/spacing"] = np.array(d.spacing)
    path = os.path.join(HERE, "raw_nd.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
