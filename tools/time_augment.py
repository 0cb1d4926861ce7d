"""Times trexhip_augment_device on the GPU: microseconds per call for 128 x 80 x 80 x {1, 3} (augmenting and the plain validation conversion), and
the augmented training step (augment + trexhip_train_step_device) beside the bare step of the same build, alternating the two in one run.
Every timed window ends in a device synchronise; every shape is warmed up first.  Writes one JSON object to profiles/time_augment.json
(--out) and prints it.
  python tools/time_augment.py [--n 128] [--pool 4096] [--calls 2000] [--steps 200] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trex_amd import capi, weights  # noqa: E402


def timed(seg, fn, count):
    seg.synchronize()
    t0 = time.perf_counter()
    for i in range(count):
        fn(i)
    seg.synchronize()
    return (time.perf_counter() - t0) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_augment.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_augment.py measures on the GPU: none here")
    W = H = 80
    p = capi.default_params(64, 64)
    p.max_batch = 1
    seg = capi.Segmenter(p)
    rng = np.random.default_rng(0)
    out = {"n": a.n, "width": W, "height": H, "pool": a.pool, "calls_per_window": a.calls, "steps_per_window": a.steps, "rounds": a.rounds, "augment": {}, "step": {}}
    for C in (1, 3):
        pool = torch.from_numpy(rng.integers(0, 256, (a.pool, H, W, C), dtype=np.uint8)).cuda()
        labels = torch.from_numpy(rng.integers(0, a.classes, a.pool).astype(np.int32)).cuda()
        x = torch.empty((a.n, H, W, C), dtype=torch.float32, device="cuda")
        y = torch.empty((a.n,), dtype=torch.int32, device="cuda")
        params = capi.default_augment_params(W, H, seed=1)
        perm = [rng.permutation(a.pool)[:a.n].astype(np.int32) for _ in range(16)]

        def augment(i, ap=params):
            seg.augment_device(pool.data_ptr(), a.pool, a.n, W, H, C, x.data_ptr(), ap=ap, indices=perm[i % 16], d_pool_targets_ptr=labels.data_ptr(),
                               d_targets_out_ptr=y.data_ptr(), counter=i)

        timed(seg, augment, 50)
        timed(seg, lambda i: augment(i, None), 50)
        aug = [timed(seg, augment, a.calls) for _ in range(a.rounds)]
        plain = [timed(seg, lambda i: augment(i, None), a.calls) for _ in range(a.rounds)]
        bytes_moved = a.n * H * W * C * 5                     # 1 byte read + 4 written per pixel-channel
        out["augment"][f"channels_{C}"] = {"augment_us_per_call": statistics.median(aug) * 1e6, "augment_us_rounds": [t * 1e6 for t in aug],
                                           "plain_us_per_call": statistics.median(plain) * 1e6, "plain_us_rounds": [t * 1e6 for t in plain],
                                           "bytes_per_call": bytes_moved, "augment_gb_per_s": bytes_moved / statistics.median(aug) / 1e9}
        # the training step with and without the loader in front of it, alternating windows of the same build
        tr = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(a.classes, 1, channels=C), a.classes, C), max_batch=a.n, lr=1e-3, seed=3)
        augment(0)

        def bare(i):
            tr.step_device(x.data_ptr(), y.data_ptr(), a.n, 0, want_loss=False)

        def augmented(i):
            augment(i)
            tr.step_device(x.data_ptr(), y.data_ptr(), a.n, 0, want_loss=False)

        timed(seg, bare, 10)
        timed(seg, augmented, 10)
        tb, ta = [], []
        for _ in range(a.rounds):
            tb.append(timed(seg, bare, a.steps))
            ta.append(timed(seg, augmented, a.steps))
        b, g = statistics.median(tb), statistics.median(ta)
        out["step"][f"channels_{C}"] = {"bare_ms_per_step": b * 1e3, "augmented_ms_per_step": g * 1e3, "bare_ms_rounds": [t * 1e3 for t in tb],
                                        "augmented_ms_rounds": [t * 1e3 for t in ta], "augmented_over_bare": g / b,
                                        "augmented_samples_per_s": a.n / g, "bare_samples_per_s": a.n / b}
        tr.close()
    seg.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
