"""The launch arithmetic of getdist_amd/csrc/binplan.hpp, on the host: the header compiles with g++ (no HIP types, the CU
count an argument), and tests/native/binplan_check.cpp compares it, exactly, with the expressions the launch sites of
binning.hip wrote out before the header existed, over the sweep F x counter bytes x B x N x CU count, and its min / max
column grouping with the former loop on 1000 random pair lists."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_binplan_equals_the_former_launch_site_expressions():
    src = os.path.join(HERE, "native", "binplan_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "binplan_check")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.split()
    # the geometry sweep alone is 2 CU counts x 8 B x 6 N x 9 F x 3 counter sizes x 6 comparisons
    assert last[-4] == "checked" and int(last[-3]) > 2 * 8 * 6 * 9 * 3 * 6 and last[-2:] == ["mismatches", "0"], r.stdout
