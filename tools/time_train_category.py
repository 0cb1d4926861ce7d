"""Times one training step (trexhip_train_step_device) of the category network -- the 3-tap mode of the one-stream exact-fp32 chain, train_arch.hip -- at
batch 32 (the reference's) and 128, 80x80x1, 4 categories, beside the same step as torch fp32 autograd + torch.optim.Adam on the same GPU
(trex_learn_category.py:18-44 restated with torch.nn; the torch step normalises its uint8-valued input as :289 does, so both sides start from the
same [0, 255] batch): device events around windows of steps, the cases alternating, the median of the windows.  Every case is warmed up first.  No
bar is set.  Writes one JSON object to profiles/train_category.json (--out) and prints it.
  python tools/time_train_category.py [--steps 20] [--windows 5]"""
import argparse
import json
import os
import statistics
import sys
import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trex_amd import capi, weights  # noqa: E402


def torch_net(categories, ch, w, h):
    """PyTorchModel restated: conv 3x3 -> BatchNorm2d -> ReLU -> pool -> element-wise Dropout(0.25), three times; fc1 -> ReLU -> Dropout -> fc2"""
    layers, ci = [], ch
    for c in weights.CATEGORY_CONVS:
        layers += [nn.Conv2d(ci, c, 3, padding=1), nn.BatchNorm2d(c), nn.ReLU(), nn.MaxPool2d(2), nn.Dropout(0.25)]
        ci = c
    return nn.Sequential(*layers, nn.Flatten(), nn.Linear(ci * (w // 8) * (h // 8), 100), nn.ReLU(), nn.Dropout(0.25), nn.Linear(100, categories))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--categories", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_category.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_train_category.py measures on the GPU: none here")
    w = h = 80
    ch = 1
    p = capi.default_params(64, 64)
    p.max_batch = 1
    seg = capi.Segmenter(p)
    rng = np.random.default_rng(0)
    blob = weights.pack_category_blob(weights.synthetic_category_state(a.categories, 1, ch, w, h), a.categories, ch, w, h)
    cases = []
    for n in a.batches:
        x = torch.from_numpy(rng.integers(0, 256, (n, h, w, ch)).astype(np.float32)).cuda()
        y = torch.from_numpy(rng.integers(0, a.categories, n).astype(np.int32)).cuda()
        tr = capi.Trainer(seg, blob, max_batch=n, lr=1e-4, seed=3)
        cases.append({"n": n, "kind": "libtrexhip, exact fp32", "tr": tr, "x": x, "y": y, "ms": []})
        net = torch_net(a.categories, ch, w, h).cuda().train()
        cases.append({"n": n, "kind": "torch fp32 autograd + Adam", "net": net, "opt": torch.optim.Adam(net.parameters(), lr=1e-4),
                      "x": x.permute(0, 3, 1, 2).contiguous(), "y": y.long(), "ms": []})
    crit = nn.CrossEntropyLoss()

    def one(c):
        if "tr" in c:
            c["tr"].step_device(c["x"].data_ptr(), c["y"].data_ptr(), c["n"], 0, want_loss=False)
        else:
            c["opt"].zero_grad(set_to_none=True)
            loss = crit(c["net"](c["x"] / 127.5 - 1), c["y"])
            loss.backward()
            c["opt"].step()

    def window(c, steps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()                                       # the context runs on torch's current stream: the events bracket exactly its steps
        for _ in range(steps):
            one(c)
        ev1.record()
        seg.synchronize()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / steps

    for c in cases:
        window(c, 3)                                       # warm-up of every case
    for _ in range(a.windows):
        for c in cases:                                    # alternating: a drift of the machine reaches every case alike
            c["ms"].append(window(c, a.steps))
    out = {"size": f"{w}x{h}", "channels": ch, "categories": a.categories, "steps_per_window": a.steps, "windows": a.windows, "cases": []}
    for c in cases:
        ms = statistics.median(c["ms"])
        out["cases"].append({"n": c["n"], "what": c["kind"], "ms_per_step": round(ms, 4), "ms_windows": [round(v, 4) for v in c["ms"]],
                             "samples_per_s": round(c["n"] / (ms * 1e-3))})
        if "tr" in c:
            c["tr"].close()
    seg.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
