"""Times track::VisualField for every individual of a batch of the C4 configuration, two ways in alternating windows of one build:
  device   trexhip_visual_field_device: every individual of every frame an observer, one call (tessellation + cast), outputs stay in HBM
  host     track::HipVisualField::cast_host, the host twin of the same rule, on one host thread (tools/time_visual_field_host.cpp)
The outlines come from trexhip_posture_auto_device on the segmented batch; the eyes are placed 2 px in front of the head point of every
outline, looking 60 degrees to either side of the tail -> head direction (VisualField::generate_eyes is the caller's; any eyes time alike).
Every GPU step is a child process under its own time limit; a step that fails or runs out of time ends the tool, nothing is started after
it.  Writes one JSON object to profiles/time_visual_field.json (--out) and prints it: microseconds per frame for each side and round, the
medians and the spread, and how many depth / id cells of the two sides differ (the device's atan2 is not libm's).
  python tools/time_visual_field.py [--config C4] [--frames 16] [--reps 5] [--rounds 5]"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_POINTS, MAX_TESS = 512, 1024


def prepare(a, path):
    """GPU step: segment, posture, build entries and observers, run the device call once, write scene + device outputs"""
    import torch
    from trex_amd import capi, synth
    fr, bg = synth.batch(a.config, a.frames)
    n, H, W = fr.shape
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=n))
    seg.set_background(bg)
    d = torch.from_numpy(fr).cuda()
    seg.segment_device(d.data_ptr(), n)
    res = seg.fetch()
    nb = sum(len(r.blobs) for r in res)
    outline = torch.zeros((nb, MAX_POINTS, 2), dtype=torch.float32, device="cuda")
    segs = torch.zeros((nb, MAX_POINTS // 2 + 1, 4), dtype=torch.float32, device="cuda")
    info = torch.zeros((nb, 8), dtype=torch.int32, device="cuda")
    seg.posture_auto_device(nb, outline.data_ptr(), segs.data_ptr(), info.data_ptr(), max_points=MAX_POINTS)
    seg.synchronize()
    h_outline = outline.cpu().numpy()
    h_info = info.cpu().numpy().view(capi.POSTURE_INFO_DTYPE).reshape(-1)
    entries, observers, offsets = [], [], [0]
    for f, r in enumerate(res):
        for k, b in enumerate(r.blobs):
            row = int(r.info["blob_begin"]) + k                 # pooled index: the posture call's row
            pos = (float(b["x0"]), float(b["y0"]))
            e = len(entries)
            entries.append((k, row, pos[0], pos[1], 0, 0))
            pi = h_info[row]
            if pi["n_outline"] > 0 and pi["tail_index"] >= 0 and pi["head_index"] >= 0:
                head, tail = h_outline[row, pi["head_index"]].astype(np.float64), h_outline[row, pi["tail_index"]].astype(np.float64)
                v = head - tail
                h = float(np.arctan2(v[1], v[0]))
                u = np.array([np.cos(h), np.sin(h)]); s = np.array([-u[1], u[0]])
                front = head + 2.0 * u + np.array(pos)
                wrap = lambda x: x - 2 * np.pi if x > np.pi else x + 2 * np.pi if x <= -np.pi else x
                observers.append((f, e, (front[0] + s[0], front[0] - s[0]), (front[1] + s[1], front[1] - s[1]),
                                  (wrap(h + np.radians(60)), wrap(h - np.radians(60)))))
        offsets.append(len(entries))
    en, ob, fe = np.array(entries, capi.VF_ENTRY_DTYPE), np.array(observers, capi.VF_OBSERVER_DTYPE), np.array(offsets, np.int32)
    max_d = float(W) ** 2 + float(H) ** 2
    got = seg.visual_field(outline.data_ptr(), info.data_ptr(), fe, en, ob, MAX_POINTS, max_tess_points=MAX_TESS, max_d=max_d)
    assert (got.status == 0).all(), np.bincount(got.status)
    with open(path, "wb") as fo:
        fo.write(struct.pack("<7i2d", 1, nb, MAX_POINTS, n, len(en), len(ob), MAX_TESS, max_d, 5.0))
        for p in (h_outline, h_info, fe, en, ob, got.depth, got.ids, got.points, got.fov, got.head_distance, got.status):
            fo.write(np.ascontiguousarray(p).tobytes())
    pts = h_info["n_outline"]
    seg.close()
    print(json.dumps({"frames": n, "entries": len(en), "observers": len(ob), "outline_points_median": float(np.median(pts[pts > 0]))}))


def device_window(a, path):
    """GPU step: the device call `reps` times on the scene of the file, outputs in HBM; prints microseconds per call"""
    import ctypes as C
    from trex_amd import capi
    with open(path, "rb") as f:
        _, nb, mp, n, ne, no, mt, max_d, md = struct.unpack("<7i2d", f.read(44))
        rd = lambda dt, cnt: np.frombuffer(f.read(np.dtype(dt).itemsize * cnt), dt, cnt)
        outline, info, fe, en, ob = rd("<f4", nb * mp * 2), rd(capi.POSTURE_INFO_DTYPE, nb), rd("<i4", n + 1), rd(capi.VF_ENTRY_DTYPE, ne), rd(capi.VF_OBSERVER_DTYPE, no)
    seg = capi.Segmenter(capi.default_params(640, 480, max_batch=1), stream=None)
    dev = []
    for x in (outline, info, fe, en, ob):
        p = seg.device_alloc(max(x.nbytes, 16)); seg.copy_to_device(p, x); dev.append(p)
    cells = no * 2 * 2 * 512
    outs = [seg.device_alloc(cells * w) for w in (8, 4, 8, 1, 8)] + [seg.device_alloc(no * 4)]
    vp = seg.default_vf_params(max_points=mp, max_tess_points=mt, max_d=max_d, max_distance=md)
    call = lambda: capi._check(capi.lib().trexhip_visual_field_device(seg.handle, C.byref(vp), *[C.c_void_p(p) for p in dev[:3]], n, C.c_void_p(dev[3]), ne,
                                                                  C.c_void_p(dev[4]), no, *[C.c_void_p(p) for p in outs]))
    call(); call()
    times = []
    for _ in range(a.reps):
        seg.synchronize()
        t0 = time.perf_counter()
        call()                                                  # the call ends with a synchronised stream
        times.append((time.perf_counter() - t0) * 1e6)
    seg.close()
    print(json.dumps(times))


def child(args, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if out.returncode != 0:
        raise SystemExit(f"step {args} failed ({out.returncode}); nothing further is started\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds every GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_visual_field.json"))
    ap.add_argument("--worker", choices=["prepare", "device"])
    ap.add_argument("--scene")
    a = ap.parse_args()
    if a.worker == "prepare":
        return prepare(a, a.scene)
    if a.worker == "device":
        return device_window(a, a.scene)
    common = ["--config", a.config, "--frames", str(a.frames), "--reps", str(a.reps)]
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene.bin")
        exe = os.path.join(tmp, "time_visual_field_host")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DTREXHIP_VF_HOST_ONLY", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "time_visual_field_host.cpp"), "-o", exe])
        meta = child(["--worker", "prepare", "--scene", scene] + common, a.step_limit)
        td, th, differ = [], [], None
        for _ in range(a.rounds):
            td.append(statistics.median(child(["--worker", "device", "--scene", scene] + common, a.step_limit)) / meta["frames"])
            line = subprocess.run([exe, scene, str(max(1, a.reps // 2))], capture_output=True, text=True, check=True).stdout.split()
            th.append(statistics.median(float(x) for x in line[:-2]) / meta["frames"])
            differ = int(line[-1])
    spread = lambda v: (max(v) - min(v)) / statistics.median(v)
    out = dict(meta, config=a.config, max_points=MAX_POINTS, max_tess_points=MAX_TESS, reps_per_window=a.reps, rounds=a.rounds,
               device_us_per_frame=statistics.median(td), host_us_per_frame=statistics.median(th), device_us_per_frame_rounds=td,
               host_us_per_frame_rounds=th, device_spread=spread(td), host_spread=spread(th), host_threads=1,
               cells_differing_depth_or_id=differ, host_over_device=statistics.median(th) / statistics.median(td))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
