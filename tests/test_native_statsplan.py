"""The launch arithmetic of getdist_amd/csrc/statsplan.hpp, on the host: the header compiles with g++ (no HIP types, the CU
count an argument), and tests/native/statsplan_check.cpp compares it, exactly, with the expressions the launch sites of
stats.hip wrote out before the header existed: the covariance plans over m x rows x CU count x weighted x two-pass forced
(with the configuration boundaries and the template arguments of the former dispatch), the block counts of the quantile
select and the lag sums, the eligibility rule of the linear quantile route, and the lag-set classification on 10 000 random
lag lists plus the sets that just miss the folded kernel.  Built with the address and undefined-behaviour sanitizers."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def test_statsplan_equals_the_former_launch_site_expressions():
    src = os.path.join(HERE, "native", "statsplan_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "statsplan_check")
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.split()
    # the covariance sweep alone is 208 slab widths x 7 row counts x 3 CU counts x 2 x 2 x 14 comparisons, the lag lists
    # 10 000 x 2 x 4
    assert last[-4] == "checked" and int(last[-3]) > 208 * 7 * 3 * 2 * 2 * 14 + 10000 * 2 * 4 and last[-2:] == ["mismatches", "0"], r.stdout
