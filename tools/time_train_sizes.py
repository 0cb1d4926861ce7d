"""Times one training step (trexhip_train_step_device) at individual_image_sizes other than 80x80 -- the generic exact-fp32 chain of
train_any.hip -- beside the 80x80 trainer in precision 1 (exact fp32 MFMA) of the same build, in one process: device events around windows of
steps, the cases alternating, the median of the windows.  Every case is warmed up first.  The figure to read is ns per MFLOP: the generic
step's should be within a small factor of the 80x80 fp32 step's; a large gap means one of the three roles of a convolution fell off the
matrix cores.  Writes one JSON object to profiles/train_sizes.json (--out) and prints it.
  python tools/time_train_sizes.py [--n 128] [--sizes 64x64,96x96,128x128] [--steps 20] [--windows 5]"""
import argparse
import json
import os
import statistics
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trex_amd import capi, weights  # noqa: E402


def flops_per_sample(w, h, ch, classes):
    """multiply-adds x 2 of one training step of V118_3: every convolution and fc1 three times (forward, data gradient, weight gradient; conv1
    has no data gradient), fc2 likewise; every pool floors"""
    c1 = 2 * 25 * ch * 16 * h * w
    c2 = 2 * 25 * 16 * 64 * (h // 2) * (w // 2)
    c3 = 2 * 25 * 64 * 128 * (h // 4) * (w // 4)
    f1 = 2 * 128 * (h // 8) * (w // 8) * 100
    return 2 * c1 + 3 * (c2 + c3 + f1 + 2 * 100 * classes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--sizes", default="64x64,96x96,128x128")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_sizes.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_train_sizes.py measures on the GPU: none here")
    p = capi.default_params(64, 64)
    p.max_batch = 1
    seg = capi.Segmenter(p)
    rng = np.random.default_rng(0)
    cases = []
    for size in a.sizes.split(",") + ["80x80"]:            # 80x80 last: the tuned trainer in precision 1, for scale
        w, h = (int(v) for v in size.split("x"))
        blob = weights.pack_blob(weights.synthetic_state(a.classes, 1, a.channels, w, h), a.classes, a.channels, w, h)
        tr = capi.Trainer(seg, blob, max_batch=a.n, lr=1e-3, seed=3, precision=1)
        x = torch.from_numpy(weights.synthetic_crops(a.n, 2, a.channels, w, h).astype(np.float32)).cuda()
        y = torch.from_numpy(rng.integers(0, a.classes, a.n).astype(np.int32)).cuda()
        cases.append({"size": f"{w}x{h}", "w": w, "h": h, "tr": tr, "x": x, "y": y, "ms": []})

    def window(c, steps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()                                       # the context runs on torch's current stream: the events bracket exactly its steps
        for _ in range(steps):
            c["tr"].step_device(c["x"].data_ptr(), c["y"].data_ptr(), a.n, 0, want_loss=False)
        ev1.record()
        seg.synchronize()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / steps

    for c in cases:
        window(c, 3)                                       # warm-up of every shape
    for _ in range(a.windows):
        for c in cases:                                    # alternating: a drift of the machine reaches every case alike
            c["ms"].append(window(c, a.steps))
    out = {"n": a.n, "channels": a.channels, "classes": a.classes, "steps_per_window": a.steps, "windows": a.windows, "cases": []}
    for c in cases:
        ms = statistics.median(c["ms"])
        mflop = a.n * flops_per_sample(c["w"], c["h"], a.channels, a.classes) / 1e6
        out["cases"].append({"size": c["size"], "chain": "80x80 precision 1" if (c["w"], c["h"]) == (80, 80) else "generic exact fp32",
                             "ms_per_step": round(ms, 4), "ms_windows": [round(v, 4) for v in c["ms"]], "samples_per_s": round(a.n / (ms * 1e-3)),
                             "mflop_per_step": round(mflop, 1), "tflops": round(mflop / ms / 1e3, 2), "ns_per_mflop": round(ms * 1e6 / mflop, 3)})
        c["tr"].close()
    seg.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
