"""
Generates tests/golden/export.npz: the files the reference GetDist writes for saveAsText / saveChainsAsText /
saveTextMetadata / writeCovMatrix / writeCorrelationMatrix (build box only: it imports the reference, which never
travels).  Inputs are regenerated on any box from seeds by tests/export_cases.py, so only reference OUTPUTS are stored
here: one uint8 array of file bytes per "<fixture>/<call>/<file name>".

    python tests/golden/make_golden_export.py
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

import export_cases  # noqa: E402

logging.getLogger().setLevel(logging.ERROR)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for fx in export_cases.fixtures():
            for call in export_cases.CALLS_FOR[fx]:
                ref = export_cases.build(MCSamples, fx)
                ref.updateBaseStatistics()  # (loadMCSamples does this; a sample set made from arrays has no covariance yet)
                for name, data in export_cases.run(ref, call, os.path.join(tmp, fx)).items():
                    out[export_cases.golden_key(fx, call, name)] = np.frombuffer(data, dtype=np.uint8)
    path = os.path.join(HERE, "export.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d files)" % (path, os.path.getsize(path), len(out)))
    for k in sorted(out):
        print("  %-60s %7d bytes" % (k, out[k].size))


if __name__ == "__main__":
    main()
