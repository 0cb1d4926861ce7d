#!/usr/bin/env python3
"""Two steps of the default bench on the GPU's own clock: every kernel and every copy kernel with its start, duration, queue and the gap in
front of it on its queue (the format of profiles/r06_c4_timeline.txt), and, per step, what lies between the end of one lane's conv3 and the
start of the next lane's conv1+conv2.

    python tools/step_timeline.py [--bench bench.py] [--steps 12] [--warmup 4] [--out FILE] [--csv kernel_trace.csv]

One `rocprofv3 --kernel-trace` run of bench.py (tracing only, no counters); --csv reads a trace that is already there.  Another build of the
library: TREXHIP_LIB_PATH, as for every A/B run; another tree's bench: --bench."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV12, CONV3 = "k_conv12_rs", "k_conv5_wpair"


def short(name):
    return name.split("(")[0].replace("trexhip::", "").replace("(anonymous namespace)::", "")[:64]


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append({"s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]), "q": r.get("Queue_Id", "?"), "name": short(r["Kernel_Name"])})
    rows.sort(key=lambda r: r["s"])
    prev = {}
    for r in rows:                          # the gap in front of a row on its queue
        r["gap"] = r["s"] - prev.get(r["q"], r["s"])
        prev[r["q"]] = r["e"]
    return rows


def networks(rows):
    """-> [(index of a network's first conv1+conv2 launch, index of its last conv3 launch)], in time order"""
    nets, first, last3 = [], None, None
    for i, r in enumerate(rows):
        if CONV12 in r["name"]:
            if first is None or last3 is not None:      # the first conv1+conv2 launch behind a conv3: the next network
                if first is not None:
                    nets.append((first, last3))
                first, last3 = i, None
        elif CONV3 in r["name"] and first is not None:
            last3 = i
    if first is not None and last3 is not None:
        nets.append((first, last3))
    return nets


def report(rows, out, steps=2):
    nets = networks(rows)
    if len(nets) < steps + 2:
        raise SystemExit("step_timeline: the trace holds %d networks, %d needed" % (len(nets), steps + 2))
    nets = nets[-(steps + 2):-1]             # (the last network's tail may be cut short by the end of the run)
    i0, i1 = max(0, nets[0][1] - 1), nets[-1][0] + 2
    t0 = rows[nets[1][0]]["s"]
    w = out.write
    w("# start_us  dur_us  gap_on_queue_us  queue  kernel\n")
    for r in rows[i0:i1]:
        w("%9.1f %8.1f %8.1f  q%-3s %s\n" % ((r["s"] - t0) / 1e3, (r["e"] - r["s"]) / 1e3, r["gap"] / 1e3, r["q"], r["name"]))
    w("#\n# from the end of the last conv3 launch of a network to the start of the next network's first %s, and what runs in between:\n" % CONV12)
    dist = []
    for (a0, a3), (b0, _) in zip(nets[:-1], nets[1:]):
        end3 = max(r["e"] for r in rows[a0:a3 + 1] if CONV3 in r["name"])
        start = rows[b0]["s"]
        dist.append((start - end3) / 1e3)
        w("#   conv3 end %9.1f (q%s) -> %s start %9.1f (q%s): %7.1f us\n" % ((end3 - t0) / 1e3, rows[a3]["q"], CONV12, (start - t0) / 1e3, rows[b0]["q"], dist[-1]))
        byq = {}
        for r in rows:
            if r["e"] > end3 and r["s"] < start and CONV3 not in r["name"]:
                byq.setdefault(r["q"], []).append(r)
        for q in sorted(byq):
            busy = sum(min(r["e"], start) - max(r["s"], end3) for r in byq[q]) / 1e3
            w("#     q%-3s %7.1f us busy: %s\n" % (q, busy, ", ".join("%s %.0f" % (r["name"].replace("void ", "")[:28], (r["e"] - r["s"]) / 1e3) for r in byq[q])))
    starts = [rows[a]["s"] for a, _ in nets]
    w("# network start to network start: %s us; conv3 end -> next %s start: mean %.1f us\n"
      % (", ".join("%.1f" % ((b - a) / 1e3) for a, b in zip(starts[:-1], starts[1:])), CONV12, sum(dist) / len(dist)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", default=os.path.join(ROOT, "bench.py"))
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--csv", default="", help="read this kernel trace instead of running the bench")
    ap.add_argument("--timeout", type=int, default=420)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    if a.csv:
        report(load(a.csv), out)
        return
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, a.bench, "--gpus", "1",
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout, cwd=d)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-4000:])
            raise SystemExit(p.returncode)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        out.write("# under the tracer: %s\n" % (line[-1][:200] if line else "(no result line)"))
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit("step_timeline: no kernel trace written")
        report(load(max(files, key=os.path.getsize)), out)


if __name__ == "__main__":
    main()
