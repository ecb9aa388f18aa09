"""
Generates tests/golden/pca.npz: MCSamples.PCA texts of the reference GetDist (build box only: it imports the reference,
which never travels).  Inputs are regenerated on any box from seeds by tests/pca_cases.py, so only reference OUTPUTS are
stored here.

    python tests/golden/make_golden_pca.py
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

import pca_cases  # noqa: E402

logging.getLogger().setLevel(logging.ERROR)


def main():
    out = {}
    for fx in pca_cases.CASES:
        ref = pca_cases.build(MCSamples, fx)
        ref.updateBaseStatistics()  # (loadMCSamples does this; a sample set made from arrays has no means yet)
        for i, kw in enumerate(pca_cases.CASES[fx]):
            key = pca_cases.case_key(fx, i)
            out[key + "/spec"] = np.array(pca_cases.case_spec(fx, i))
            r = ref.PCA(**kw)
            out[key + "/text"] = np.array(pca_cases.as_text(r))
            out[key + "/kind"] = np.array("str" if isinstance(r, str) else "list%d" % len(r))
    path = os.path.join(HERE, "pca.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
