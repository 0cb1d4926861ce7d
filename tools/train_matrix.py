"""Runs a matrix of training cases that reaches every chain of the trainers (dev tool, needs the GPU): V118_3 at 80x80 with 1 and 3 channels and
both precisions, V118_3 at 21x13x3 (the size-following convolutions, every level with an odd edge), v100, v110 and the category network at 21x13x3
and 80x80x1, and V118_3 at 80x80x1 with batches of 1 and of 67 (ragged sample tiles of fc1 and its data gradient).  Every case but the last two uses
a batch of 8 = max_batch; all use 5 classes and fixed seeds.  Per case: two steps with the library's own masks, one with injected masks, one step
that the device refuses (a target equal to `classes`) with a good step queued behind it, one more good step, one evaluation and one prediction of
11 crops.

   python tools/train_matrix.py OUT.bin

OUT.bin holds, per case and one after the other, the exported blob, every tensor's gradient and Adam moments (trexhip_trainer_read, kinds 1..3),
the returned losses / correct counts, the step counts and the probabilities; OUT.bin.json their names and offsets, and the refusal's text.  Two
builds of the library (TREXHIP_LIB_PATH) compute the same thing when the files are byte-identical.  The training counterpart of
tools/identify_matrix.py."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trex_amd import capi, weights

CLASSES = 5
PREDICT = 11
# (architecture, W, H, channels, precision, batch)
CASES = (("v118_3", 80, 80, 1, 0, 8), ("v118_3", 80, 80, 1, 1, 8), ("v118_3", 80, 80, 3, 0, 8), ("v118_3", 21, 13, 3, 0, 8),
         ("v100", 21, 13, 3, 0, 8), ("v100", 80, 80, 1, 0, 8), ("v110", 80, 80, 1, 0, 8),
         ("category", 21, 13, 3, 0, 8), ("category", 80, 80, 1, 0, 8),
         ("v118_3", 80, 80, 1, 0, 1), ("v118_3", 80, 80, 1, 0, 67))


def batch(n, seed, W, H, CH):
    """float32 NHWC inputs in [0, 255] (blobs on black, rescaled: not integers) and labels"""
    rng = np.random.default_rng(seed)
    x = weights.synthetic_crops(n, seed + 7, CH, W, H).astype(np.float32)
    x = np.clip(x * rng.uniform(0.85, 1.15, (n, 1, 1, 1)).astype(np.float32) + rng.uniform(0.0, 3.0, x.shape).astype(np.float32) * (x > 0), 0.0, 255.0)
    return np.ascontiguousarray(x, np.float32), rng.integers(0, CLASSES, n).astype(np.int32)


def main():
    out_path = sys.argv[1]
    index, out = [], open(out_path, "wb")

    def put(case, what, arr, **extra):
        b = np.ascontiguousarray(arr).tobytes()
        index.append(dict({"case": case, "what": what, "offset": out.tell(), "bytes": len(b)}, **extra))
        out.write(b)

    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    for (arch, W, H, CH, precision, n) in CASES:
        name = f"{arch} {W}x{H}x{CH} precision {precision} batch {n}"
        if arch == "category":
            shapes = weights.category_shapes(CLASSES, CH, W, H)
            blob = weights.pack_category_blob(weights.synthetic_category_state(CLASSES, 31, CH, W, H), CLASSES, CH, W, H)
        else:
            shapes = weights.shapes(CLASSES, CH, W, H, arch)
            blob = weights.pack_blob(weights.synthetic_state(CLASSES, 31, CH, W, H, arch), CLASSES, CH, W, H, arch)
        tr = capi.Trainer(seg, blob, max_batch=n, lr=1e-3, seed=17, precision=precision)
        scalars, steps = [], []

        def step(seed, masks=None, targets=None, want_loss=True):
            x, y = batch(n, seed, W, H, CH)
            dx = torch.from_numpy(x).cuda()
            dy = torch.from_numpy(y if targets is None else targets).cuda()
            dm = torch.from_numpy(masks).cuda() if masks is not None else None
            r = tr.step_device(dx.data_ptr(), dy.data_ptr(), n, dm.data_ptr() if dm is not None else 0, want_loss=want_loss)
            if r is not None:
                scalars.extend(r)
            steps.append(tr.steps)

        step(40)
        step(41)
        step(42, masks=(np.random.default_rng(5).random(n * tr.mask_row) >= 0.1).astype(np.uint8))
        # a class index out of range in device memory: the device refuses that step and the one queued behind it, the next synchronising call says so
        bad = batch(n, 43, W, H, CH)[1].copy()
        bad[n // 2] = CLASSES
        step(43, targets=bad, want_loss=False)
        refused = ""
        try:
            step(44)
        except capi.TrexHipError as e:
            refused = str(e)
        steps.append(tr.steps)
        step(45)                                              # the trainer goes on where it was
        x, y = batch(n, 46, W, H, CH)
        dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        scalars.extend(tr.evaluate_device(dx.data_ptr(), dy.data_ptr(), n))
        crops = torch.from_numpy(weights.synthetic_crops(PREDICT, 47, CH, W, H)).cuda()
        probs = torch.zeros((PREDICT, CLASSES), dtype=torch.float32, device="cuda")
        tr.predict_device(crops.data_ptr(), PREDICT, probs.data_ptr())
        seg.synchronize()
        put(name, "blob", np.frombuffer(tr.export(), np.uint8))
        for kind, letter in ((1, "G"), (2, "M"), (3, "V")):
            for i, (tensor, shp) in enumerate(shapes):
                put(name, f"{letter} {tensor}", tr.read(i, kind, shp))
        put(name, "scalars", np.array(scalars, np.float64))
        put(name, "steps", np.array(steps, np.int64), refused=refused)
        put(name, "probs", probs.cpu().numpy())
        tr.close()
        print(f"{name}: steps {steps[-1]}, refused: {bool(refused)}", flush=True)
    seg.close()
    out.close()
    with open(out_path + ".json", "w") as f:
        json.dump(index, f, indent=0)
    print(f"{len(CASES)} cases, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
