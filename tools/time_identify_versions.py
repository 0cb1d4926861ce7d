"""Times trexhip_identify_device for each of the five identity networks (v118_3, v100, v110, v119, v200) at 80x80x1, 100 classes, on 6400
resident crops, under FP32 and FP16X3, and beside each the same network as torch.nn.functional fp32 on the same GPU (PyTorch-ROCm's own
convolutions, the layer table of tests/vi_arch_ref.py) -- a yardstick, not a gate.  Writes profiles/identify_versions.json.

Per (version, mode): windows of `reps` calls, the library's and torch's alternating, after a warm-up of both; the medians of the windows;
crops/s; algorithmic FLOP per crop from the layer table (2 x multiply-adds of the reference's layers) -> TFLOP/s and the fraction of the matching
matrix peak (FP16X3: 2.5 PF dense fp16 -- the mode spends three piece products per product; FP32: 157.3 TF); the shares of conv2 and conv3 in
the call from trexhip_profile_* in a run of its own (first layer, further convolutions, pools and tail are the rest).  This is a whole-call
rate over peak, not a kernel's share of peak.
  python tools/time_identify_versions.py [--crops 6400] [--reps 3] [--windows 5] [--versions v118_3,v100,...] [--out profiles/identify_versions.json]"""
import argparse
import json
import os
import statistics
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from trex_amd import capi, weights  # noqa: E402
import vi_arch_ref  # noqa: E402

PEAK = {"fp16x3": 2.5e15, "fp32": 157.3e12}        # MI355X dense fp16 / fp32 matrix peak, FLOP/s
MODES = {"fp32": capi.CNN_FP32, "fp16x3": capi.CNN_FP16X3}
STAGE_CONV2, STAGE_CONV3, STAGE_CNN_ALL = 2, 3, 4
TORCH_BATCH = 256                                  # torch walks the crops in batches of this many (v200 holds 7.6 MB of activations per crop)


def flops_per_crop(arch, w, h, ch, classes):
    L = vi_arch_ref.V118_3 if arch == "v118_3" else weights.ARCH_LAYERS[arch]
    fl, ci = 0, ch
    for i, (co, k) in enumerate(L["convs"], 1):
        fl += 2 * k * k * ci * co * h * w
        ci = co
        if arch == "v200":
            if i in (2, 4, 5):
                h, w = h // 3, w // 3
        else:
            h, w = h // 2, w // 2
    flat = ci if arch == "v200" else ci * h * w
    return fl + 2 * flat * L["hidden"] + 2 * L["hidden"] * classes


def timed(fn, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / reps


def write(path, records):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "note": "whole-call rates; torch_fp32 is PyTorch-ROCm's own convolutions on the same crops, a yardstick",
                   "records": records}, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=6400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--versions", default="v118_3,v100,v110,v119,v200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identify_versions.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is measured without one"
    w = h = 80
    n = a.crops
    records = []
    for arch in a.versions.split(","):
        st = weights.synthetic_state(a.classes, 1, 1, w, h, arch=arch)
        seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
        seg.load_weights(weights.pack_blob(st, a.classes, 1, w, h, arch=arch))
        base = torch.from_numpy(weights.synthetic_crops(256, 2, 1, w, h)).cuda()      # 256 distinct crops, tiled
        crops = base.repeat((n + 255) // 256, 1, 1, 1)[:n].contiguous()
        probs = torch.empty((n, a.classes), dtype=torch.float32, device="cuda")
        t = {k: torch.from_numpy(v).cuda() for k, v in st.items()}

        def run_torch():
            with torch.no_grad():
                for c0 in range(0, n, TORCH_BATCH):
                    x = crops[c0:c0 + TORCH_BATCH].float().permute(0, 3, 1, 2)
                    torch.softmax(vi_arch_ref.forward_tensors(t, x, arch), 1)

        fl = flops_per_crop(arch, w, h, 1, a.classes)
        for mname, mode in MODES.items():
            seg.set_identity_precision(mode)
            run_lib = lambda: seg.identify_device(crops.data_ptr(), n, probs.data_ptr())
            for _ in range(2):
                run_lib(); run_torch()
            torch.cuda.synchronize()
            lib_ms, torch_ms = [], []
            for _ in range(a.windows):                     # alternating windows: both see the same neighbours on the machine
                lib_ms.append(timed(run_lib, a.reps))
                torch_ms.append(timed(run_torch, a.reps))
            guard = list(seg.guard_stats())
            seg.profile_enable(True); seg.profile_reset()  # the stage shares, in a run of their own
            for _ in range(a.reps):
                run_lib()
            seg.synchronize()
            st_ms = {k: seg.profile_read(s)[0] for k, s in (("conv2", STAGE_CONV2), ("conv3", STAGE_CONV3), ("all", STAGE_CNN_ALL))}
            seg.profile_enable(False)
            ms, tms = statistics.median(lib_ms), statistics.median(torch_ms)
            cps = n / (ms * 1e-3)
            rec = {"version": arch, "size": f"{w}x{h}x1", "classes": a.classes, "mode": mname, "crops": n, "chunk_crops": seg.identify_chunk_crops(),
                   "ms_per_call_median": round(ms, 4), "ms_per_call_windows": [round(x, 4) for x in lib_ms], "crops_per_s": round(cps),
                   "mflop_per_crop": round(fl / 1e6, 2), "tflops_algorithmic": round(cps * fl / 1e12, 2), "peak": mname + " matrix",
                   "share_of_peak_whole_call": round(cps * fl / PEAK[mname], 5),
                   "share_conv2": round(st_ms["conv2"] / st_ms["all"], 4) if st_ms["all"] else None,
                   "share_conv3": round(st_ms["conv3"] / st_ms["all"], 4) if st_ms["all"] else None, "guard": guard,
                   "torch_fp32_ms_median": round(tms, 4), "torch_fp32_ms_windows": [round(x, 4) for x in torch_ms], "torch_batch": TORCH_BATCH,
                   "torch_fp32_crops_per_s": round(n / (tms * 1e-3)), "speed_against_torch_fp32": round(tms / ms, 3)}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            write(a.out, records)                          # after every record: a run that is cut short keeps what it measured
        seg.close()
        del crops, probs, base, t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
