"""Times the categorisation of a batch of crops that are in HBM, two ways in alternating windows of one build:
  A  trexhip_categorize_device + trexhip_tracklet_labels_device (the category network, k_cat_label, the vote), per arithmetic mode
  B  the same network restated in torch float32 eager on the same GPU (trex_learn_category.py:18-44 in eval mode on x / 127.5 - 1) + argmax, then
     the labels copied to the host and voted there with numpy (what TRex does with the labels it receives)
Workload: 25 600 crops of 80 x 80 x 1, 4 categories, 256 tracklets (100 rows each, interleaved); synthetic weights and crops.
Device times are taken with device events around the calls of a window; the host vote of B with the host clock, reported on its own and in B's sum.
A's vote returns a host value (the skipped count), so its time includes that round trip.  Every GPU step is a child process under its own time
limit; a step that fails or runs out of time ends the tool, nothing is started after it.  Writes one JSON object to profiles/time_categorize.json
(--out) and prints it: the medians of `rounds` alternating windows in milliseconds, every window's value, and the spread.
  python tools/time_categorize.py [--crops 25600] [--reps 5] [--rounds 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = H = 80
CH, CATEGORIES, TRACKLETS = 1, 4, 256
MODES = {"FP16X3": 3, "FP32": 0}


def workload(a):
    from trex_amd import weights
    st = weights.synthetic_category_state(CATEGORIES, 21, CH, W, H)
    crops = weights.synthetic_crops(256, 22, CH, W, H)
    crops = np.ascontiguousarray(np.tile(crops, (-(-a.crops // 256), 1, 1, 1))[:a.crops])
    tracklet = (np.arange(a.crops) % TRACKLETS).astype(np.int32)
    return st, crops, tracklet


def device_window(a):
    """GPU step: call A `reps` times in mode a.mode; prints milliseconds per call and the labels' histogram"""
    import torch
    from trex_amd import capi, weights
    st, crops, tracklet = workload(a)
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_category_weights(weights.pack_category_blob(st, CATEGORIES, CH, W, H))
    seg.set_identity_precision(MODES[a.mode])
    n = len(crops)
    d_crops, d_tr = torch.from_numpy(crops).cuda(), torch.from_numpy(tracklet).cuda()
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    counts = torch.zeros((TRACKLETS, CATEGORIES), dtype=torch.int32, device="cuda")
    rows, label = torch.zeros(TRACKLETS, dtype=torch.int32, device="cuda"), torch.zeros(TRACKLETS, dtype=torch.int32, device="cuda")

    def call():
        seg.categorize_device(d_crops.data_ptr(), n, lab.data_ptr())
        seg.tracklet_labels_device(lab.data_ptr(), d_tr.data_ptr(), n, TRACKLETS, CATEGORIES, counts.data_ptr(), rows.data_ptr(), label.data_ptr())
    call(); call()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); call(); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    out = dict(ms=times, labels=np.bincount(lab.cpu().numpy(), minlength=CATEGORIES).tolist(), tracklet_labels=label.cpu().numpy().tolist())
    seg.close()
    print(json.dumps(out))


def torch_window(a):
    """GPU step: call B `reps` times; prints milliseconds per call (device part, host vote) and the labels' histogram"""
    import torch
    import torch.nn.functional as F
    st, crops, tracklet = workload(a)
    t = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    n = len(crops)
    d_crops = torch.from_numpy(crops).cuda()

    def net():
        with torch.no_grad():
            x = (d_crops.to(torch.float32) / 127.5 - 1).permute(0, 3, 1, 2)
            for i in (1, 2, 3):
                x = F.conv2d(x, t[f"conv{i}.weight"], t[f"conv{i}.bias"], padding=1)
                x = F.batch_norm(x, t[f"batch_norm{i}.running_mean"], t[f"batch_norm{i}.running_var"], t[f"batch_norm{i}.weight"], t[f"batch_norm{i}.bias"],
                                 training=False, eps=1e-5)
                x = F.max_pool2d(F.relu(x), 2, 2)
            x = F.relu(F.linear(x.reshape(n, -1), t["fc1.weight"], t["fc1.bias"]))
            return torch.softmax(F.linear(x, t["fc2.weight"], t["fc2.bias"]), dim=1).argmax(dim=1)

    def vote(labels):
        counts = np.zeros((TRACKLETS, CATEGORIES), np.uint32)
        ok = (labels >= 0) & (labels < CATEGORIES)
        np.add.at(counts, (tracklet[ok], labels[ok]), 1)
        return np.where(counts.max(1) > 0, counts.argmax(1), -1)
    net(); net()
    dev, host = [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); lab = net(); e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        label = vote(lab.cpu().numpy())
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    print(json.dumps(dict(ms=dev, host_vote_ms=host, labels=np.bincount(lab.cpu().numpy(), minlength=CATEGORIES).tolist(), tracklet_labels=label.tolist())))


def child(args, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        raise SystemExit(f"step {args} failed ({out.returncode}); nothing further is started\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=25600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds every GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_categorize.json"))
    ap.add_argument("--worker", choices=["device", "torch"])
    ap.add_argument("--mode", default="FP16X3", choices=sorted(MODES))
    a = ap.parse_args()
    if a.worker == "device":
        return device_window(a)
    if a.worker == "torch":
        return torch_window(a)
    common = ["--crops", str(a.crops), "--reps", str(a.reps)]
    ta, tb, tbh = {m: [] for m in MODES}, [], []
    agree = {}
    for _ in range(a.rounds):
        b = child(["--worker", "torch"] + common, a.step_limit)
        tb.append(statistics.median(b["ms"])); tbh.append(statistics.median(b["host_vote_ms"]))
        for m in MODES:
            d = child(["--worker", "device", "--mode", m] + common, a.step_limit)
            ta[m].append(statistics.median(d["ms"]))
            agree[m] = dict(label_histogram_equal=d["labels"] == b["labels"], tracklet_labels_equal=d["tracklet_labels"] == b["tracklet_labels"])
    med = statistics.median
    spread = lambda v: (max(v) - min(v)) / med(v)
    out = dict(crops=a.crops, size=[W, H, CH], categories=CATEGORIES, tracklets=TRACKLETS, reps_per_window=a.reps, rounds=a.rounds,
               torch_ms=med(tb) + med(tbh), torch_device_ms=med(tb), torch_host_vote_ms=med(tbh), torch_device_ms_rounds=tb, torch_spread=spread(tb), agreement=agree)
    for m in MODES:
        out[f"device_{m}_ms"] = med(ta[m]); out[f"device_{m}_ms_rounds"] = ta[m]; out[f"device_{m}_spread"] = spread(ta[m])
        out[f"torch_over_device_{m}"] = out["torch_ms"] / med(ta[m])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
