"""Times one end-of-epoch validation of identity training on the GPU, at the reference's proportions (16 classes x 400 validation crops for
the per-class accuracy, 200 frames x 16 crops for the uniqueness estimate), two ways in alternating windows of one build:
  resident   Trainer.predict_device + Segmenter.validation_metrics, twice (trexhip_train_predict_device, trexhip_validation_metrics_device)
  exported   what there was before: Trainer.export -> Segmenter.load_weights -> identify_device -> copy the rows to the host -> NumPy
Every timed window ends with host values in hand (both paths synchronise by themselves); both are warmed up first.  Writes one JSON object
to profiles/time_validation.json (--out) and prints it.
  python tools/time_validation.py [--classes 16] [--per-class 400] [--frames 200] [--reps 20] [--rounds 5]"""
import argparse
import json
import math
import os
import statistics
import sys
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trex_amd import capi, weights  # noqa: E402

NORMAL = np.float32(1) + np.float32(math.exp(-float(np.float32(math.pi))))


def host_metrics(val_rows, val_targets, uni_rows, ranges, classes):
    """the host loop: plot_comparison_raw's column 3 and Accumulation::calculate_uniqueness's third value, in NumPy"""
    hit = np.bincount(val_targets[val_rows.argmax(axis=1) == val_targets], minlength=classes)
    count = np.bincount(val_targets, minlength=classes)
    acc = np.divide(hit, count, out=np.zeros(classes), where=count > 0)
    pos = np.where(uni_rows > 0, uni_rows, np.float32(0))
    ids = pos.argmax(axis=1)
    max_p = pos[np.arange(len(pos)), ids]
    percentages = 0.0
    for a, b in ranges:
        best = np.zeros(classes, np.float32)
        np.maximum.at(best, ids[a:b], max_p[a:b])
        seen = best > 0
        distinct = int(seen.sum())
        p = float(np.float32(distinct) / np.float32(b - a)) if b > a else 0.0
        if distinct:
            accum = np.float32(0)
            for v in best[seen]:
                accum = np.float32(accum + v)
            p = 1.0 / (1.0 + math.exp(-float(np.float32(accum / np.float32(distinct))) * math.pi)) * float(NORMAL) * p
        percentages += p
    return acc, float(np.float32(percentages / len(ranges)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--per-class", type=int, default=400)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--max-batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_validation.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_validation.py measures on the GPU: none here")
    classes, nv, nu = a.classes, a.classes * a.per_class, a.frames * a.classes
    p = capi.default_params(64, 64)
    p.max_batch = 1
    seg = capi.Segmenter(p)
    tr = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(classes, 1), classes), max_batch=a.max_batch, lr=1e-3, seed=3)
    val_y = np.repeat(np.arange(classes), a.per_class).astype(np.int32)
    d_val = torch.from_numpy(weights.synthetic_crops(nv, 2)).cuda()
    d_uni = torch.from_numpy(weights.synthetic_crops(nu, 3)).cuda()
    d_val_y = torch.from_numpy(val_y).cuda()
    ranges = np.array([(classes * k, classes * (k + 1)) for k in range(a.frames)], np.int32)
    d_probs = torch.empty((max(nv, nu), classes), dtype=torch.float32, device="cuda")

    def resident():
        tr.predict_device(d_val.data_ptr(), nv, d_probs.data_ptr())
        acc = seg.validation_metrics(d_probs.data_ptr(), nv, classes, d_targets_ptr=d_val_y.data_ptr()).per_class_accuracy
        tr.predict_device(d_uni.data_ptr(), nu, d_probs.data_ptr())
        return acc, seg.validation_metrics(d_probs.data_ptr(), nu, classes, frame_ranges=ranges).mean_unique

    def exported():
        seg.load_weights(tr.export())
        seg.identify_device(d_val.data_ptr(), nv, d_probs.data_ptr())
        val_rows = seg.copy_to_host(d_probs.data_ptr(), (nv, classes), np.float32)
        seg.identify_device(d_uni.data_ptr(), nu, d_probs.data_ptr())
        uni_rows = seg.copy_to_host(d_probs.data_ptr(), (nu, classes), np.float32)
        return host_metrics(val_rows, val_y, uni_rows, ranges, classes)

    def timed(fn):
        seg.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        seg.synchronize()
        return (time.perf_counter() - t0) / a.reps

    r, e = resident(), exported()                              # warm-up, and the two paths agree (different arithmetic of the network: 1e-4 rows)
    agree = {"max_abs_accuracy_difference": float(np.abs(r[0] - e[0]).max()), "uniqueness_resident": r[1], "uniqueness_exported": e[1]}
    resident(); exported()
    tr_, te_ = [], []
    for _ in range(a.rounds):
        tr_.append(timed(resident))
        te_.append(timed(exported))
    out = {"classes": classes, "validation_crops": nv, "frames": a.frames, "uniqueness_crops": nu, "max_batch": a.max_batch, "reps_per_window": a.reps,
           "rounds": a.rounds, "resident_us": statistics.median(tr_) * 1e6, "exported_us": statistics.median(te_) * 1e6,
           "resident_us_rounds": [t * 1e6 for t in tr_], "exported_us_rounds": [t * 1e6 for t in te_],
           "exported_over_resident": statistics.median(te_) / statistics.median(tr_), "agreement": agree}
    tr.close(); seg.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
