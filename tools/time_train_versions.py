"""Times one training step (trexhip_train_step_device) of the identity networks v100 and v110 -- the generic exact-fp32 chain of train_arch.hip --
at batch 128, 80x80x1, 100 classes, beside the V118_3 trainer in precision 1 (exact fp32 MFMA) of the same build and beside the same step as
torch fp32 autograd + torch.optim.Adam on the same GPU (the architectures restated with torch.nn, as time_identify_versions.py does for
inference): device events around windows of steps, the cases alternating, the median of the windows.  Every case is warmed up first.  No bar is
set.  Writes one JSON object to profiles/train_versions.json (--out) and prints it.
  python tools/time_train_versions.py [--n 128] [--steps 20] [--windows 5]"""
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


def torch_net(arch, classes, ch, w, h):
    """visual_identification_network_torch.py:184-382 restated: the order of pool, norm and ReLU and the dropout rates are each version's own"""
    co = (16, 64, 128 if arch == "v118_3" else 100)
    layers, ci = [], ch
    for c in co:
        conv = nn.Conv2d(ci, c, 5, padding="same")
        if arch == "v100":
            layers += [conv, nn.ReLU(), nn.MaxPool2d(2), nn.Dropout2d(0.25)]
        elif arch == "v110":
            layers += [conv, nn.MaxPool2d(2), nn.BatchNorm2d(c), nn.ReLU(), nn.Dropout2d(0.25)]
        else:
            layers += [conv, nn.BatchNorm2d(c), nn.ReLU(), nn.MaxPool2d(2), nn.Dropout2d(0.05)]
        ci = c
    layers += [nn.Flatten(), nn.Linear(ci * (w // 8) * (h // 8), 100)]
    layers += {"v100": [nn.ReLU(), nn.Dropout(0.5)], "v110": [nn.BatchNorm1d(100), nn.ReLU(), nn.Dropout(0.25)], "v118_3": [nn.LayerNorm(100), nn.ReLU(), nn.Dropout(0.05)]}[arch]
    return nn.Sequential(*layers, nn.Linear(100, classes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_versions.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_train_versions.py measures on the GPU: none here")
    w = h = 80
    ch = 1
    p = capi.default_params(64, 64)
    p.max_batch = 1
    seg = capi.Segmenter(p)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(0.0, 255.0, (a.n, h, w, ch)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, a.classes, a.n).astype(np.int32)).cuda()
    x_nchw, y64 = x.permute(0, 3, 1, 2).contiguous(), y.long()
    cases = []
    for arch in ("v100", "v110", "v118_3"):
        blob = weights.pack_blob(weights.synthetic_state(a.classes, 1, ch, w, h, arch), a.classes, ch, w, h, arch)
        tr = capi.Trainer(seg, blob, max_batch=a.n, lr=1e-5, seed=3, precision=1)
        cases.append({"name": arch, "kind": "libtrexhip, exact fp32", "tr": tr, "ms": []})
        net = torch_net(arch, a.classes, ch, w, h).cuda().train()
        cases.append({"name": arch, "kind": "torch fp32 autograd + Adam", "net": net, "opt": torch.optim.Adam(net.parameters(), lr=1e-5), "ms": []})
    crit = nn.CrossEntropyLoss()

    def one(c):
        if "tr" in c:
            c["tr"].step_device(x.data_ptr(), y.data_ptr(), a.n, 0, want_loss=False)
        else:
            loss = crit(c["net"](x_nchw), y64)
            loss.backward()
            c["opt"].step()
            c["opt"].zero_grad(set_to_none=True)

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
    out = {"n": a.n, "size": f"{w}x{h}", "channels": ch, "classes": a.classes, "steps_per_window": a.steps, "windows": a.windows, "cases": []}
    for c in cases:
        ms = statistics.median(c["ms"])
        out["cases"].append({"version": c["name"], "what": c["kind"], "ms_per_step": round(ms, 4), "ms_windows": [round(v, 4) for v in c["ms"]],
                             "samples_per_s": round(a.n / (ms * 1e-3))})
        if "tr" in c:
            c["tr"].close()
    seg.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
