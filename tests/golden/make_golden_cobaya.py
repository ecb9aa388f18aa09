"""
Generates tests/golden/cobaya.json by importing the REAL GetDist (the reference; build container only): what it makes of the
Cobaya runs of tests/cobaya_cases.py (yamls committed under tests/golden/cobaya/, chain numbers generated from a seed):

1. per run the reference can load: the loaded sample set (cobaya_cases.summarize: names, labels, derived flags, renames,
   str(ranges), sampler, label, temperature, properties, rows, chain offsets, a sample row, bounds by name, means);
2. per yaml: the results of the cobaya_interface functions (cobaya_cases.interface_results);
3. get_range on cobaya_cases.RANGE_CASES.

The file holds strings and numbers only.  Running this again gives the same file.

    python tests/golden/make_golden_cobaya.py
"""

import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("GETDIST_REFERENCE", "/root/reference"))

from getdist import cobaya_interface as ci  # noqa: E402  (the reference)
from getdist import loadMCSamples  # noqa: E402

import cobaya_cases as cc  # noqa: E402


def main():
    out = dict(runs={}, interface={}, get_range=cc.range_results(ci))
    with tempfile.TemporaryDirectory() as tmp:
        for name, run in cc.RUNS.items():
            out["interface"][name] = cc.interface_results(ci, name, os.path.join(tmp, "interface"))
            if name not in cc.LOADED_RUNS:
                continue
            root = cc.build_run(name, os.path.join(tmp, "load"))
            mc = loadMCSamples(root, no_cache=True, settings={"ignore_rows": run["ignore_rows"]})
            exact, numbers = cc.summarize(mc)
            out["runs"][name] = dict(exact=exact, numbers=numbers)
            print("%-6s %2d parameters, %4d rows, offsets %s, sampler %s, properties %s"
                  % (name, len(exact["names"]), exact["numrows"], exact["chain_offsets"], exact["sampler"], exact["properties"]))
    a = out["runs"]["runA"]["exact"]  # what the issue states of run A
    assert a["names"] == ["a", "b", "th", "c", "d", "chi2", "chi2__gauss_like"], a["names"]
    assert a["numrows"] == 280 and a["chain_offsets"] == [0, 140, 280]
    assert a["ranges_upper"]["a"] == 3.0 and a["ranges_upper"]["fixedp"] == 0.06 and a["ranges_lower"]["b"] is None
    path = os.path.join(HERE, "cobaya.json")
    with open(path, "w", encoding="utf-8") as f:
        f.write(cc.compact_json(out) + "\n")
    print("wrote cobaya.json (%d bytes)" % os.path.getsize(path))


if __name__ == "__main__":
    main()
