"""Compares the kernel traces of two runs of the same program (dev tool): the library's launches of each run in the order they started, as
(kernel name, grid, workgroup, LDS bytes).  The runs launched the same thing when the two sequences are equal.
   rocprofv3 --kernel-trace --output-format csv -d DIR_A -- python tools/identify_matrix.py ...      (once per build, TREXHIP_LIB_PATH)
   python tools/compare_kernel_traces.py DIR_A DIR_B [OUT.json]"""
import collections
import csv
import glob
import json
import os
import sys


def launches(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (d, files)
    rows = [r for r in csv.DictReader(open(files[0])) if "trexhip" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cols = lambda prefix: sorted(c for c in rows[0] if c.startswith(prefix))
    gcols, wcols, lcols = cols("Grid_Size"), cols("Workgroup_Size"), cols("LDS")
    assert gcols and wcols and len(lcols) == 1, sorted(rows[0])
    return [(r["Kernel_Name"], tuple(int(r[c]) for c in gcols), tuple(int(r[c]) for c in wcols), int(r[lcols[0]])) for r in rows]


a, b = launches(sys.argv[1]), launches(sys.argv[2])
first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
doc = {"launches": [len(a), len(b)], "equal": a == b, "first_difference": None if first is None else {"index": first, "a": a[first], "b": b[first]},
       "kernels": dict(sorted(collections.Counter(k[0].split("(")[0] for k in a).items()))}
print(json.dumps({k: doc[k] for k in ("launches", "equal", "first_difference")}))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(doc, f, indent=1)
sys.exit(0 if a == b else 1)
