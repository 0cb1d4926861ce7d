"""Times the last step of the output_tracklet_images export -- one median image per tracklet (Export.cpp:1287-1364) -- on a crop pool that is
resident in HBM: 25 600 crops of 80x80 in 256 tracklets of 100, gray and colour, and 8 tracklets of 3200 (gray); three ways, the first two in
alternating windows of one build:
  device   Segmenter.tracklet_medians (trexhip_tracklet_medians_device): the pool is reduced where it is, tracklets x H x W bytes come back
  host     a fair host route: copy_to_host of the whole pool, then per tracklet the gray conversion and np.partition(stack, m // 2, axis=0)[m // 2]
           -- the value the walk over the final histogram gives -- so the host side is not held back by the interpreter
  twin     what the reference does today, after the same copy: hist_utils::addImage per image, line by line (track::tracklet_images_host, C++,
           one thread), on --twin-tracklets tracklets and scaled to all of them (it needs minutes otherwise); timed once
Every timed window ends with host values in hand.  All routes are warmed up first and their results compared byte for byte.  Also reports the
device call's time as a multiple of its HBM time (pool bytes + output bytes over 8 TB/s).  Writes one JSON object to
profiles/time_tracklet_medians.json (--out) and prints it.
  python tools/time_tracklet_medians.py [--reps 10] [--rounds 5] [--twin-tracklets 8]"""
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
from trex_amd import capi  # noqa: E402

HBM_BYTES_PER_S = 8e12
WORKLOADS = [("gray", 256, 100, 1), ("colour", 256, 100, 3), ("long", 8, 3200, 1)]      # name, tracklets, crops per tracklet, channels
W = H = 80


def build_twin(tmp):
    so = os.path.join(tmp, "libtime_tracklet_medians_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "time_tracklet_medians_host.cpp"), "-o", so])
    h = C.CDLL(so)
    h.ttm_host_twin.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    h.ttm_host_twin.restype = C.c_double
    return h


def host_medians(pool, per, T):
    """pool uint8 (n, H, W, C), tracklet t = rows [t * per, (t + 1) * per)"""
    out = np.empty((T, H, W), np.uint8)
    for t in range(T):
        stack = pool[t * per:(t + 1) * per]
        if stack.shape[-1] == 3:
            c = stack.astype(np.uint32)
            stack = ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)
        else:
            stack = stack[..., 0]
        out[t] = np.partition(stack, per // 2, axis=0)[per // 2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--twin-tracklets", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_tracklet_medians.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tracklet_medians.py measures on the GPU: none here")
    p = capi.default_params(64, 64)
    p.max_batch = 1
    seg = capi.Segmenter(p)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        twin = build_twin(tmp)
        for name, T, per, ch in WORKLOADS:
            n = T * per
            rng = np.random.default_rng(n + ch)
            # crops as the export sees them: a blob of noisy gray values on a dark background, moving a little from image to image
            pool = np.zeros((n, H, W, ch), np.uint8)
            yy, xx = np.mgrid[0:H, 0:W]
            for i in range(0, n, 512):
                m = min(512, n - i)
                cy, cx = rng.normal(40, 3, (2, m, 1, 1))
                inside = ((yy - cy) ** 2 / 200.0 + (xx - cx) ** 2 / 900.0) < 1.0
                pool[i:i + m] = (inside[..., None] * rng.integers(40, 220, (m, H, W, ch))).astype(np.uint8)
            tracklet = np.repeat(np.arange(T, dtype=np.int32), per)
            d_pool, d_tr = torch.from_numpy(pool).cuda(), torch.from_numpy(tracklet).cuda()

            def device():
                return seg.tracklet_medians(d_pool.data_ptr(), n, W, H, ch, d_tr.data_ptr(), T)[0]

            def host():
                return host_medians(seg.copy_to_host(d_pool.data_ptr(), pool.shape, np.uint8), per, T)

            def timed(fn, reps):
                seg.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                seg.synchronize()
                return (time.perf_counter() - t0) / reps

            d, h = device(), host()                             # warm-up, and the routes agree
            same = d.tobytes() == h.tobytes()
            tt = min(a.twin_tracklets, T)
            twin_out = np.zeros((tt, H, W), np.uint8)
            twin_s = twin.ttm_host_twin(pool.ctypes.data_as(C.c_void_p), n, W, H, ch, per, tt, twin_out.ctypes.data_as(C.c_void_p))
            same_twin = twin_s >= 0 and twin_out.tobytes() == d[:tt].tobytes()
            device(); host()
            td, th = [], []
            for _ in range(a.rounds):
                td.append(timed(device, a.reps))
                th.append(timed(host, max(1, a.reps // 5)))
            copy_s = timed(lambda: seg.copy_to_host(d_pool.data_ptr(), pool.shape, np.uint8), 3)
            dev, hst = statistics.median(td), statistics.median(th)
            hbm_s = (pool.nbytes + T * H * W) / HBM_BYTES_PER_S
            results.append({"workload": name, "tracklets": T, "crops_per_tracklet": per, "channels": ch, "crops": n, "pool_bytes": pool.nbytes,
                            "device_us": dev * 1e6, "host_us": hst * 1e6, "host_over_device": hst / dev,
                            "device_us_rounds": [t * 1e6 for t in td], "host_us_rounds": [t * 1e6 for t in th],
                            "pool_copy_to_host_us": copy_s * 1e6, "hbm_us": hbm_s * 1e6, "device_over_hbm": dev / hbm_s,
                            "twin_tracklets_timed": tt, "twin_s_timed": twin_s, "twin_s_scaled_to_all": twin_s * T / tt,
                            "twin_plus_copy_over_device": (twin_s * T / tt + copy_s) / dev,
                            "same_bytes_host": same, "same_bytes_twin": same_twin, "bytes_to_host_device": T * H * W + 4 * T})
    seg.close()
    out = {"width": W, "height": H, "reps_per_window": a.reps, "rounds": a.rounds, "workloads": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    if not all(r["same_bytes_host"] and r["same_bytes_twin"] for r in results):
        raise SystemExit("the routes disagree")


if __name__ == "__main__":
    main()
