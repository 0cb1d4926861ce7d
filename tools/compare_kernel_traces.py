"""Compares the kernel traces of two runs of the same program (dev tool): the library's launches of each run in the order they started, as
(kernel name, grid, workgroup, LDS bytes).  The runs launched the same thing when the two sequences are equal.
   rocprofv3 --kernel-trace --output-format csv -d DIR_A -- python tools/identify_matrix.py ...      (once per build, TREXHIP_LIB_PATH)
   python tools/compare_kernel_traces.py DIR_A DIR_B [OUT.json] [--multiset] [--map REGEX=REPLACEMENT ...]
--multiset compares how often each (kernel, grid, workgroup, LDS bytes) was launched and not the order: a program that forks onto a second stream
(the V118_3 trainer at 80x80) starts its kernels in an order that differs from run to run.  The kernel is then named k_...<...> without its
namespace and signature, and every --map rewrites the names of DIR_A first: a kernel that was renamed between the builds is compared with its
namesake.  OUT.json then also holds the median duration per kernel name of both runs, in microseconds."""
import collections
import csv
import glob
import json
import os
import re
import statistics
import sys

args = sys.argv[1:]
multiset = "--multiset" in args
maps = [args[i + 1].split("=", 1) for i, a in enumerate(args) if a == "--map"]
pos = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--map")]


def short(name, renames=()):
    m = re.search(r"k_\w+(<[^>]*>)?", name)
    s = m.group(0) if m else name
    for pat, rep in renames:
        s = re.sub(pat, rep, s)
    return s


def launches(d, renames=()):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (d, files)
    rows = [r for r in csv.DictReader(open(files[0])) if "trexhip" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cols = lambda prefix: sorted(c for c in rows[0] if c.startswith(prefix))
    gcols, wcols, lcols = cols("Grid_Size"), cols("Workgroup_Size"), cols("LDS")
    assert gcols and wcols and len(lcols) == 1, sorted(rows[0])
    name = (lambda r: short(r["Kernel_Name"], renames)) if multiset else (lambda r: r["Kernel_Name"])
    us = collections.defaultdict(list)
    for r in rows:
        us[name(r)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [(name(r), tuple(int(r[c]) for c in gcols), tuple(int(r[c]) for c in wcols), int(r[lcols[0]])) for r in rows], us


(a, us_a), (b, us_b) = launches(pos[0], maps), launches(pos[1])
if multiset:
    ca, cb = collections.Counter(a), collections.Counter(b)
    equal = ca == cb
    first = None if equal else {"only_a": [list(k) + [v] for k, v in (ca - cb).items()], "only_b": [list(k) + [v] for k, v in (cb - ca).items()]}
else:
    equal = a == b
    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    first = None if i is None else {"index": i, "a": a[i], "b": b[i]}
doc = {"launches": [len(a), len(b)], "equal": equal, "first_difference": first,
       "kernels": dict(sorted(collections.Counter(k[0].split("(")[0] for k in a).items()))}
if multiset:
    doc["median_us"] = {k: [round(statistics.median(us_a[k]), 2) if k in us_a else None, round(statistics.median(us_b[k]), 2) if k in us_b else None]
                        for k in sorted(set(us_a) | set(us_b))}
print(json.dumps({k: doc[k] for k in ("launches", "equal", "first_difference")}))
if len(pos) > 2:
    with open(pos[2], "w") as f:
        json.dump(doc, f, indent=1)
sys.exit(0 if equal else 1)
