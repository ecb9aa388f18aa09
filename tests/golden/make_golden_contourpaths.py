"""
Writes tests/golden/contourpaths.npz: contourpy's contour lines (canonicalised: closed lines rotated to their smallest
vertex, lines sorted) and filled(level, inf) areas for the cases of tests/contourpath_cases.py with sides up to 64, the
contourpy version, and the largest difference from the oracle measured while writing.

    python tests/golden/make_golden_contourpaths.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import contourpath_cases as cc  # noqa: E402


def main():
    import contourpy

    from getdist_amd.contourpaths import ContourPaths

    orc = cc.oracle_of_cases()
    names, crcs, task_case, task_level, task_line_off = [], [], [], [], [0]
    line_off, line_closed, xy, areas = [0], [], [], []
    worst_abs = worst_ulp = worst_area = 0.0
    for ci, c in enumerate(cc.golden_cases()):
        names.append(c["name"])
        crcs.append(cc.case_crc(c))
        mine = ContourPaths(c["x"], c["y"], c["levels"], orc[c["name"]])
        for k, (lines, area) in enumerate(cc.contourpy_reference(c)):
            ref = cc.canonical_lines(lines)
            a, u = cc.compare_lines(cc.canonical_lines(mine.lines(k)), ref, c, "%s level %d" % (c["name"], k))
            worst_abs, worst_ulp = max(worst_abs, a), max(worst_ulp, u)
            worst_area = max(worst_area, abs(mine.area(k) - area))
            task_case.append(ci)
            task_level.append(k)
            for closed, pts in ref:
                line_closed.append(closed)
                xy.append(pts)
                line_off.append(line_off[-1] + len(pts))
            task_line_off.append(len(line_closed))
            areas.append(area)
    out = os.path.join(HERE, "contourpaths.npz")
    np.savez_compressed(
        out, case_names=np.array(names), case_crc=np.array(crcs, dtype=np.uint32), task_case=np.array(task_case, dtype=np.int32),
        task_level=np.array(task_level, dtype=np.int32), task_line_off=np.array(task_line_off, dtype=np.int64),
        line_off=np.array(line_off, dtype=np.int64), line_closed=np.array(line_closed, dtype=bool),
        xy=np.concatenate(xy) if xy else np.zeros((0, 2)), area=np.array(areas), contourpy_version=np.array(contourpy.__version__),
        max_abs_diff=np.array(worst_abs), max_ulp_diff=np.array(worst_ulp), max_area_diff=np.array(worst_area))
    print("%s: %d cases, %d tasks, %d lines, %d vertices, %d bytes; contourpy %s; oracle within %.3g (%.2f ulp of the larger edge "
          "end), areas within %.3g" % (out, len(names), len(areas), len(line_closed), line_off[-1], os.path.getsize(out),
                                       contourpy.__version__, worst_abs, worst_ulp, worst_area))


if __name__ == "__main__":
    main()
