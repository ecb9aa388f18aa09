"""
Generates tests/golden/single_samples.npz: the rows, arrays and file texts of the reference GetDist's
MCSamples.makeSingleSamples / random_single_samples_indices (build box only: it imports the reference, which never
travels).  Inputs are regenerated on any box from seeds by tests/single_cases.py, so only reference OUTPUTS are stored here.

    python tests/golden/make_golden_single.py
"""

import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
if os.environ.get("GETDIST_REFERENCE"):  # a checkout of the reference GetDist (else the installed getdist)
    sys.path.insert(0, os.environ["GETDIST_REFERENCE"])

from getdist import MCSamples  # noqa: E402  (the reference)

import single_cases  # noqa: E402

logging.getLogger().setLevel(logging.ERROR)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for fx in single_cases.fixtures():
            ref = single_cases.build(MCSamples, fx)
            ref.updateBaseStatistics()  # (loadMCSamples does this; a sample set made from arrays has no norm yet)
            for call in single_cases.CALLS_FOR[fx]:
                r = single_cases.run(ref, call, tmp)
                out["%s/%s" % (fx, call)] = np.array(r) if isinstance(r, str) else np.asarray(r)
    path = os.path.join(HERE, "single_samples.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
