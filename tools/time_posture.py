"""Time of whole posture calls on the bench scene (dev tool): the single pass (k_posture + the walk kernels) and the retry entry point, at
max_points 256 and 512.  Per quantity: device time per call from a pair of events around a fixed number of calls, and the host's time in the
same calls (the enqueue for the single pass; the retry entry point waits for its rounds, so its host time is the whole call).  One JSON line.
   PYTHONPATH=. python tools/time_posture.py [frames] [--calls K] [--dump DIR]
--dump DIR: also write outline / segments / info of one single-pass and one retry call (max_points 256, zeroed buffers) as .npy files, to
compare two builds of the library byte for byte (TREXHIP_LIB_PATH selects the build)."""
import argparse, json, os, time
import numpy as np, torch
from trex_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("frames", nargs="?", type=int, default=64)
ap.add_argument("--calls", type=int, default=400)
ap.add_argument("--dump", default=None)
a = ap.parse_args()

n = a.frames
W = H = 2048
base, bg = synth.batch_torch("C4", 8, "cuda")
frames = base.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
seg = capi.Segmenter(capi.default_params(W, H, max_batch=n, max_blobs=256))
seg.set_background(bg if not isinstance(bg, np.ndarray) else bg)
seg.segment_device(frames.data_ptr(), n)
res = seg.fetch()
nb = sum(len(r.blobs) for r in res)


def buffers(MP):
    return (torch.zeros((nb, MP, 2), dtype=torch.float32, device="cuda"), torch.zeros((nb, MP // 2 + 1, 4), dtype=torch.float32, device="cuda"),
            torch.zeros((nb, 8), dtype=torch.int32, device="cuda"))


def calls(MP):
    o, s4, inf = buffers(MP)
    single = lambda: seg.posture_device(nb, o.data_ptr(), s4.data_ptr(), inf.data_ptr(), max_points=MP)
    auto = lambda: seg.posture_auto_device(nb, o.data_ptr(), s4.data_ptr(), inf.data_ptr(), max_points=MP)
    return single, auto, (o, s4, inf)


def timed(fn, k):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); e0.record()
    for _ in range(k):
        fn()
    e1.record(); t1 = time.perf_counter()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / k, 1e6 * (t1 - t0) / k


out = {"blobs": nb, "calls": a.calls}
for MP in (256, 512):
    single, auto, keep = calls(MP)
    out[f"single_{MP}_gpu_us"], out[f"single_{MP}_host_us"] = timed(single, a.calls)
    out[f"auto_{MP}_gpu_us"], out[f"auto_{MP}_host_us"] = timed(auto, a.calls)
    if MP == 256:
        i = keep[2].cpu().numpy()
        ok = i[:, 0] == 0
        out["mean_traced"], out["mean_outline"], out["mean_segments"] = float(i[ok, 5].mean()), float(i[ok, 1].mean()), float(i[ok, 2].mean())
if a.dump:
    os.makedirs(a.dump, exist_ok=True)
    # a frame's place in the blob pool differs from run to run: rows in frame order
    order = np.concatenate([int(r.info["blob_begin"]) + np.arange(len(r.blobs)) for r in res])
    for name in ("single", "auto"):
        single, auto, (o, s4, inf) = calls(256)
        (single if name == "single" else auto)()
        seg.synchronize()
        for what, t in (("outline", o), ("segments", s4), ("info", inf)):
            np.save(os.path.join(a.dump, f"{name}_{what}.npy"), t.cpu().numpy()[order])
print(json.dumps(out))
