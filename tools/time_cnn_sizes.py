"""Times trexhip_identify_device at individual_image_size other than 80x80 (the generic chain, cnn_any.hip) on resident crops:
device-event time per call after warm-up, crops/s, algorithmic TFLOP/s from the shapes and the share of the 2.5 PF dense fp16 peak.
80x80 (the tuned chain) is listed beside them for comparison.  One JSON line per case.
  python tools/time_cnn_sizes.py [--crops 25600] [--reps 5] [--sizes 64x64,96x96,128x128,80x80] [--modes fp16x3,fp32]"""
import argparse
import json
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trex_amd import capi, weights  # noqa: E402

PEAK_FP16 = 2.5e15        # MI355X dense fp16 matrix peak, FLOP/s
MODES = {"fp32": capi.CNN_FP32, "bf16x6": capi.CNN_BF16X6, "bf16x3": capi.CNN_BF16X3, "fp16x3": capi.CNN_FP16X3}


def flops_per_crop(w, h, ch, classes):
    """multiply-adds x 2 of V118_3 as the reference defines it (5x5 'same' convolutions, every pool floors)"""
    conv = 2 * 25 * (ch * 16 * h * w + 16 * 64 * (h // 2) * (w // 2) + 64 * 128 * (h // 4) * (w // 4))
    return conv + 2 * 128 * (h // 8) * (w // 8) * 100 + 2 * 100 * classes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=25600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--sizes", default="64x64,96x96,128x128,80x80")
    ap.add_argument("--modes", default="fp16x3,fp32")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    for size in a.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        st = weights.synthetic_state(a.classes, 1, a.channels, w, h)
        seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
        seg.load_weights(weights.pack_blob(st, a.classes, a.channels, w, h))
        base = torch.from_numpy(weights.synthetic_crops(256, 2, a.channels, w, h)).cuda()      # 256 distinct crops, tiled
        reps = (a.crops + 255) // 256
        crops = base.repeat(reps, 1, 1, 1)[:a.crops].contiguous()
        probs = torch.empty((a.crops, a.classes), dtype=torch.float32, device="cuda")
        for mname in a.modes.split(","):
            seg.set_identity_precision(MODES[mname])
            for _ in range(a.warmup):
                seg.identify_device(crops.data_ptr(), a.crops, probs.data_ptr())
            seg.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            # the context runs on torch's current stream (capi.Segmenter default): the events bracket exactly its calls
            ev0.record()
            for _ in range(a.reps):
                seg.identify_device(crops.data_ptr(), a.crops, probs.data_ptr())
            ev1.record()
            seg.synchronize()
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1) / a.reps
            fl = flops_per_crop(w, h, a.channels, a.classes)
            cps = a.crops / (ms * 1e-3)
            rec = {"size": f"{w}x{h}", "channels": a.channels, "mode": mname, "crops": a.crops, "ms_per_call": round(ms, 4),
                   "crops_per_s": round(cps), "mflop_per_crop": round(fl / 1e6, 2), "tflops": round(cps * fl / 1e12, 1),
                   "share_of_fp16_peak": round(cps * fl / PEAK_FP16, 4), "guard": list(seg.guard_stats())}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
        seg.close()
        del crops, probs, base
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
