"""A/B of two builds of the library on timing commands (dev tool): alternating processes, one unrecorded run of each first, then `reps` recorded
runs of each; every process has its own time limit and nothing is started after a failure.  A command is a script of this repository with its
arguments that prints one JSON line whose timed quantities end in _us (or are named by --quantity); several commands are separated by `--`
and their quantities share one table.  Writes values / median / min / max per build and quantity and whether the branch's median lies inside
the parent's min .. max (the parent build is the yardstick).
   python tools/ab_time.py PARENT_LIB OUT.json REPS [--quantity NAME] -- tools/time_posture.py 64 --calls 400 [-- tools/time_identify.py --graphs 0]"""
import json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
parent_lib, out_path, reps = os.path.abspath(sys.argv[1]), sys.argv[2], int(sys.argv[3])
rest, commands, extra = sys.argv[4:], [], []
if rest[0] == "--quantity":
    extra, rest = [rest[1]], rest[2:]
for a in rest:
    if a == "--":
        commands.append([])
    else:
        commands[-1].append(a)
libs = {"parent": parent_lib, "branch": os.path.join(ROOT, "trex_amd", "libtrexhip.so")}
runs = {"parent": [], "branch": []}
for rep in range(reps + 1):
    for build in ("parent", "branch"):
        env = dict(os.environ, TREXHIP_LIB_PATH=libs[build], PYTHONPATH=ROOT)
        r = {}
        for cmd in commands:
            p = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"{build} run {rep} of {cmd} failed ({p.returncode}): {p.stderr[-2000:]}")
            r.update(json.loads(p.stdout.strip().splitlines()[-1]))
        print(build, rep, r, flush=True)
        if rep > 0:
            runs[build].append(r)
quantities = [k for k, v in runs["parent"][0].items() if (k.endswith("_us") or k in extra) and isinstance(v, (int, float))]
doc = {"commands": [" ".join(c) for c in commands], "repetitions": reps, "order": "alternating, one process per run, after one unrecorded run of each"}
for build in runs:
    doc[build] = {}
    for q in quantities:
        v = [r[q] for r in runs[build]]
        doc[build][q] = {"values": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
doc["branch_median_inside_parent_range"] = {q: doc["parent"][q]["min"] <= doc["branch"][q]["median"] <= doc["parent"][q]["max"] for q in quantities}
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc["branch_median_inside_parent_range"]))
