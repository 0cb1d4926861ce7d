"""A/B of two builds of the library on tools/time_posture.py (dev tool): alternating processes, one unrecorded run of each first, then `reps` recorded
runs of each; every process has its own time limit and nothing is started after a failure.  Writes values / median / min / max per build and
quantity and whether the branch's median lies inside the parent's min .. max (the parent build is the yardstick).
   python tools/ab_time_posture.py PARENT_LIB OUT.json [reps]"""
import json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
parent_lib, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
CMD = ["tools/time_posture.py", "64", "--calls", "400"]
libs = {"parent": parent_lib, "branch": os.path.join(ROOT, "trex_amd", "libtrexhip.so")}
runs = {"parent": [], "branch": []}
for rep in range(reps + 1):
    for build in ("parent", "branch"):
        env = dict(os.environ, TREXHIP_LIB_PATH=libs[build], PYTHONPATH=ROOT)
        p = subprocess.run([sys.executable] + CMD, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        if p.returncode != 0:
            sys.exit(f"{build} run {rep} failed ({p.returncode}): {p.stderr[-2000:]}")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        print(build, rep, r, flush=True)
        if rep > 0:
            runs[build].append(r)
quantities = [k for k in runs["parent"][0] if k.endswith("_us")]
doc = {"command": " ".join(CMD), "repetitions": reps, "order": "alternating, one process per run, after one unrecorded run of each", "blobs": runs["parent"][0]["blobs"]}
for build in runs:
    doc[build] = {}
    for q in quantities:
        v = [r[q] for r in runs[build]]
        doc[build][q] = {"values": v, "median": statistics.median(v), "min": min(v), "max": max(v)}
doc["branch_median_inside_parent_range"] = {q: doc["parent"][q]["min"] <= doc["branch"][q]["median"] <= doc["parent"][q]["max"] for q in quantities}
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc["branch_median_inside_parent_range"]))
