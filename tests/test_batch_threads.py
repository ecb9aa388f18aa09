"""
The choreography of gd_density2d_batch (getdist_amd/csrc/batch2d.hpp) as a stand-alone program over C++ stubs
(tests/native/batch_threads_main.cpp), under ThreadSanitizer and under AddressSanitizer + UBSan: four shapes of a call,
then the largest shape with one fault per run -- a stub that fails or throws in the binning thread, the shear chain,
the staging thread, the finisher or the enqueuer.  Every run is a child process with a time limit: a run that does not
end (a wait nobody releases, a thread nobody tells to stop) is what this test exists to catch.  Plain executables; nothing
is loaded into this interpreter.
"""

import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

RUN_SECONDS = 10  # a run takes well under a second; its longest bounded wait is 90 ms


@pytest.fixture(scope="module")
def programs():
    import build_threads

    return build_threads.programs()


@pytest.mark.parametrize("kind", ["thread", "address"])
def test_every_hand_off_ends_and_frees_its_blocks(programs, kind):
    exe = programs[kind]
    runs = subprocess.run([exe, "list"], capture_output=True, text=True, timeout=RUN_SECONDS, check=True).stdout.split()
    assert runs[0] == "shapes" and len(runs) == 15, runs
    for name in ("fused-binning", "second-binning", "sheared-histograms", "second-stage-a", "first-get-h", "convolution",
                 "build-batch-alloc"):
        assert any(r.startswith(name) and r.endswith(("throws", "throw")) for r in runs), name
    for run in runs:
        try:
            r = subprocess.run([exe, run], capture_output=True, text=True, timeout=RUN_SECONDS)
        except subprocess.TimeoutExpired:
            pytest.fail("%s under -fsanitize=%s did not end within %d s" % (run, kind, RUN_SECONDS))
        assert r.returncode == 0, (run, r.stdout[-2000:] + r.stderr[-4000:])
        assert r.stderr == "", (run, r.stderr[-4000:])  # (a sanitizer's report goes to stderr)
        assert r.stdout.strip() == run + ": passed", (run, r.stdout)
