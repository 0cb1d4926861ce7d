"""Times Tracker::prefilter's blob policy on one loaded batch of the C4 configuration on the GPU, two ways in alternating windows of one
build:
  device   trexhip_prefilter_device (re-threshold + decisions + presumed_nr, everything stays in HBM)
  host     what there was before: trexhip_rethreshold_device -> trexhip_fetch_rethreshold -> the policy on one host thread
           (track::HipPrefilter::host_policy, tools/time_prefilter_host.cpp) -> upload of presumed_nr for the split search
Both start behind trexhip_fetch on the loaded batch and every timed window ends with a synchronised stream.  The per-frame counts of the
two routes must agree.  Writes one JSON object to profiles/time_prefilter.json (--out) and prints it.
  python tools/time_prefilter.py [--config C4] [--frames 16] [--reps 10] [--rounds 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trex_amd import capi, synth  # noqa: E402


def build_host_route(tmp):
    so = os.path.join(tmp, "libtime_prefilter_host.so")
    lib_dir = os.path.join(ROOT, "trex_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "time_prefilter_host.cpp"), "-o", so, "-L", lib_dir, "-ltrexhip", "-Wl,-rpath," + lib_dir])
    capi.lib()                                                 # libtrexhip is loaded first: the shim binds to the same copy
    h = C.CDLL(so)
    h.tp_prepare.argtypes = [C.c_void_p]
    h.tp_host_route.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                C.c_double, C.c_void_p, C.c_void_p]
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--track-threshold", type=int, default=25)
    ap.add_argument("--track-threshold-2", type=int, default=40)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_prefilter.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_prefilter.py measures on the GPU: none here")
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
    loaded = ld.fetch()
    total = sum(len(r.blobs) for r in loaded)
    cm = float(ld.params.cm_per_pixel)
    med = float(np.median(np.concatenate([r.blobs["n_pixels"] for r in loaded]))) * cm * cm
    ranges = np.array([(0.6 * med, 1.4 * med)], np.float64)    # around the median blob: committed, big and OutsideRange all occur
    ratio = (0.2, 2.0)
    bg_c = np.ascontiguousarray(bg)

    with tempfile.TemporaryDirectory() as tmp:
        host_lib = build_host_route(tmp)
        assert host_lib.tp_prepare(ld._h) == 0
        pf = capi.Prefilter(ld, n, total)
        d_presumed_host = ld.device_alloc(4 * max(total, 1))
        host_counts = np.zeros((n, 3), np.int32)

        def device():
            pf.run(a.track_threshold, 0, [tuple(r) for r in ranges], a.track_threshold_2, ratio)

        def host():
            rc = host_lib.tp_host_route(ld._h, a.track_threshold, 0, a.track_threshold_2, ratio[0], ratio[1], ranges.ctypes.data, len(ranges),
                                        bg_c.ctypes.data, W, cm, d_presumed_host, host_counts.ctypes.data)
            assert rc == 0, rc

        def timed(fn):
            ld.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            ld.synchronize()
            return (time.perf_counter() - t0) / a.reps

        device(); host()                                       # warm-up, and the two routes agree
        got = pf.fetch()
        assert np.array_equal(got.counts[:, :3], host_counts) and (got.counts[:, 3] == 0).all(), (got.counts, host_counts)
        assert np.array_equal(got.presumed_nr, ld.copy_to_host(d_presumed_host, (total,), np.int32))
        device(); host()
        td, th = [], []
        for _ in range(a.rounds):
            td.append(timed(device))
            th.append(timed(host))
        out = {"config": a.config, "frames": n, "detect_blobs": total, "track_threshold": a.track_threshold, "track_threshold_2": a.track_threshold_2,
               "size_range_cm2": ranges.tolist(), "committed": int(got.counts[:, 0].sum()), "big": int(got.counts[:, 1].sum()),
               "filtered_out": int(got.counts[:, 2].sum()), "reps_per_window": a.reps, "rounds": a.rounds,
               "device_us": statistics.median(td) * 1e6, "host_us": statistics.median(th) * 1e6,
               "device_us_rounds": [t * 1e6 for t in td], "host_us_rounds": [t * 1e6 for t in th],
               "host_over_device": statistics.median(th) / statistics.median(td)}
        pf.close(); ld.device_free(d_presumed_host)
    det.close(); ld.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
