"""Times trexhip_load_frames_v6_device on the GPU beside the detect pass on the same frames: 256 frames of the C4 configuration are
segmented and packed once; then, in alternating windows of one build,
  load     Segmenter.load_frames_v6_device on the packed bodies (a second context with the same parameters)
  detect   Segmenter.segment_device on the frames the bodies came from
Neither window fetches: both calls only enqueue, the window ends with a stream synchronise.  Both are warmed up first, and the loaded
tables are compared with the segmented ones before anything is timed.  Writes one JSON object to profiles/time_load_frames.json
(--out) and prints it.
  python tools/time_load_frames.py [--config C4] [--frames 256] [--reps 20] [--rounds 5]"""
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
from trex_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_load_frames.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_load_frames.py measures on the GPU: none here")
    fr, bg = synth.batch(a.config, a.frames)
    n, H, W = fr.shape
    det, ld = capi.Segmenter(capi.default_params(W, H, max_batch=n)), capi.Segmenter(capi.default_params(W, H, max_batch=n))
    det.set_background(bg); ld.set_background(bg)
    d_frames = torch.from_numpy(fr).cuda()
    det.segment_device(d_frames.data_ptr(), n)
    res = det.fetch()
    cap = sum(11 + 4 * len(r.blobs) + 4 * len(r.runs) + len(r.pixels) for r in res) + 64
    d_bodies = torch.zeros(cap, dtype=torch.uint8, device="cuda"); d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    det.pack_frames_v6_device(d_bodies.data_ptr(), cap, d_off.data_ptr())
    det.synchronize()
    ld.load_frames_v6_device(d_bodies.data_ptr(), d_off.data_ptr(), n)
    for x, y in zip(res, ld.fetch()):
        assert x.blobs.tobytes() == y.blobs.tobytes() and x.runs.tobytes() == y.runs.tobytes() and x.pixels.tobytes() == y.pixels.tobytes()

    def load():
        ld.load_frames_v6_device(d_bodies.data_ptr(), d_off.data_ptr(), n)

    def detect():
        det.segment_device(d_frames.data_ptr(), n)

    def timed(fn, seg):
        seg.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        seg.synchronize()
        return (time.perf_counter() - t0) / a.reps

    load(); detect(); ld.synchronize(); det.synchronize()
    tl, td = [], []
    for _ in range(a.rounds):
        tl.append(timed(load, ld))
        td.append(timed(detect, det))
    out = {"config": a.config, "frames": n, "width": W, "height": H, "blobs": int(sum(len(r.blobs) for r in res)),
           "lines": int(sum(len(r.runs) for r in res)), "pixels": int(sum(len(r.pixels) for r in res)), "body_bytes": int(d_off.cpu().numpy()[n]),
           "reps_per_window": a.reps, "rounds": a.rounds, "load_us": statistics.median(tl) * 1e6, "detect_us": statistics.median(td) * 1e6,
           "load_us_rounds": [t * 1e6 for t in tl], "detect_us_rounds": [t * 1e6 for t in td],
           "load_over_detect": statistics.median(tl) / statistics.median(td)}
    det.close(); ld.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
