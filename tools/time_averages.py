"""Times VINetwork::paverages on rows that are resident in HBM -- what Accumulation::check_additional_range asks for once per candidate
range -- at 100 individuals x 100 classes and 25 600 and 102 400 rows, two ways in alternating windows of one build:
  device   Segmenter.class_averages (trexhip_class_averages_device): the rows are reduced where they are, individuals x classes floats come back
  host     what there was before: copy_to_host of all rows, then the loop of paverages on the host.  Here the loop is NumPy -- per
           individual np.add.reduce over its rows along axis 0, which adds row after row in float32 like the reference's std::transform --
           so the host side is not held back by the interpreter
Every timed window ends with host values in hand (both paths synchronise by themselves); both are warmed up first, and their results are
compared byte for byte.  Writes one JSON object to profiles/time_averages.json (--out) and prints it.
  python tools/time_averages.py [--ids 100] [--classes 100] [--rows 25600 102400] [--reps 20] [--rounds 5]"""
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
from trex_amd import capi  # noqa: E402


def host_paverages(rows, keys, n_ids):
    samples = np.bincount(keys, minlength=n_ids).astype(np.float32)
    values = np.zeros((n_ids, rows.shape[1]), np.float32)
    order = np.argsort(keys, kind="stable")
    starts = np.concatenate([[0], np.cumsum(samples.astype(np.int64))])
    grouped = rows[order]
    for k in range(n_ids):
        if samples[k] > 0:
            values[k] = np.add.reduce(grouped[starts[k]:starts[k + 1]], axis=0, dtype=np.float32) / samples[k]
    return samples, values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=100)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--rows", type=int, nargs="+", default=[25600, 102400])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_averages.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_averages.py measures on the GPU: none here")
    p = capi.default_params(64, 64)
    p.max_batch = 1
    seg = capi.Segmenter(p)
    results = []
    for n in a.rows:
        rng = np.random.default_rng(n)
        rows = rng.random((n, a.classes)).astype(np.float32) ** 8
        rows = (rows / rows.sum(axis=1, keepdims=True)).astype(np.float32)
        keys = rng.integers(0, a.ids, n).astype(np.int32)
        d_rows, d_keys = torch.from_numpy(rows).cuda(), torch.from_numpy(keys).cuda()

        def device():
            m = seg.class_averages(d_rows.data_ptr(), n, a.classes, d_keys.data_ptr(), a.ids)
            return m.samples, m.values

        def host():
            return host_paverages(seg.copy_to_host(d_rows.data_ptr(), (n, a.classes), np.float32), keys, a.ids)

        def timed(fn):
            seg.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            seg.synchronize()
            return (time.perf_counter() - t0) / a.reps

        d, h = device(), host()                                 # warm-up, and the two routes agree
        same = d[0].tobytes() == h[0].tobytes() and d[1].tobytes() == h[1].tobytes()
        device(); host()
        td, th = [], []
        for _ in range(a.rounds):
            td.append(timed(device))
            th.append(timed(host))
        results.append({"rows": n, "device_us": statistics.median(td) * 1e6, "host_us": statistics.median(th) * 1e6,
                        "device_us_rounds": [t * 1e6 for t in td], "host_us_rounds": [t * 1e6 for t in th],
                        "host_over_device": statistics.median(th) / statistics.median(td), "same_bytes": same,
                        "bytes_to_host_device": 4 * a.ids * (a.classes + 3) + 16, "bytes_to_host_host": 4 * n * a.classes})
    seg.close()
    out = {"ids": a.ids, "classes": a.classes, "reps_per_window": a.reps, "rounds": a.rounds, "sizes": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
