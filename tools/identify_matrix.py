"""Runs a matrix of identify_device cases that reaches every chain of the identity network's forward pass (dev tool, needs the GPU):
80x80 with 1 and 3 channels, 64x64, 100x60 and 120x16 (the 8-, 4- and 16-wide tiles of the any-size chain), one small case of each of v100, v110,
v119, v200 and the category network, the four precision modes, crop counts on both sides of every launch threshold, the chain-selecting
values of TREXHIP_CONV_GEOM, aligned and unaligned crop pointers, one case per chain that trips the fp16 range guard, and one default
12800-crop batch.  Every case is called four times, so that with graphs on the chain is run directly, captured and replayed.

   python tools/identify_matrix.py OUT.bin [--graphs 0]

OUT.bin holds the probabilities and logits of every case one after the other, OUT.bin.json their names and offsets.  Two builds of the library
(TREXHIP_LIB_PATH) compute the same thing when the files are byte-identical; under a kernel trace (one traced process per build) they launch the
same thing when the sequences of (kernel name, grid, workgroup, LDS bytes) are equal: tools/compare_kernel_traces.py."""
import json
import os
import sys

if "--graphs" in sys.argv:
    os.environ["TREXHIP_GRAPHS"] = sys.argv[sys.argv.index("--graphs") + 1]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trex_amd import capi, weights

CLASSES = 8
MODES = (capi.CNN_FP32, capi.CNN_BF16X6, capi.CNN_BF16X3, capi.CNN_FP16X3)
COUNTS = (1, 100, 1024, 1025, 3199, 3200)
GEOMS = (0, 1 << 28, 1 << 29, 1 << 30, 2048)
ARCH_CASES = (("v100", 69, 13, 1), ("v110", 37, 35, 1), ("v119", 45, 43, 3), ("v200", 55, 29, 1), ("category", 100, 14, 1))


def out_of_range(st):
    """every crop's conv1 output leaves the fp16 range, later layers stay finite (tests/test_cnn_gpu.py)"""
    st = {k: v.copy() for k, v in st.items()}
    st["conv1.weight"] *= 4000.0
    st["bn1.running_var"] = np.full(16, 1.0, np.float32); st["bn1.running_mean"] = np.zeros(16, np.float32)
    st["bn2.running_var"] = np.full(64, 1e10, np.float32)
    return st


def arch_out_of_range(st, category):
    """the first layer's output leaves the fp16 range; the second convolution (category: the first BatchNorm's scale alone, as
    tests/test_categorize_gpu.py) takes the factor back"""
    st = {k: v.copy() for k, v in st.items()}
    if category:
        st["batch_norm1.weight"] = (st["batch_norm1.weight"] * 3e5).astype(np.float32)
    else:
        st["conv1.weight"] *= 4000.0; st["conv1.bias"] *= 4000.0
        st["conv2.weight"] /= 4000.0
    return st


def main():
    out_path = sys.argv[1]
    index, blob = [], open(out_path, "wb")
    nmax = 12800
    rng = np.random.default_rng(3)
    pool = torch.from_numpy(rng.integers(0, 256, nmax * 80 * 80 + 64, dtype=np.uint8)).cuda()       # crops of every case: a window of this
    real = {ch: torch.from_numpy(np.concatenate([weights.synthetic_crops(5, 77, channels=ch).reshape(-1), np.zeros(64, np.uint8)])).cuda() for ch in (1, 3)}
    probs = torch.empty((nmax, CLASSES), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    labels = torch.empty(nmax, dtype=torch.int32, device="cuda")

    def run(seg, name, src, n, cb, mode, aligned, category=False):
        base = src.data_ptr() + (16 - src.data_ptr() % 16) % 16 + (0 if aligned else 3)
        assert n * cb + 19 <= src.numel()
        seg.set_identity_precision(mode)
        for _ in range(4):
            if category:
                seg.categorize_device(base, n, labels.data_ptr(), probs.data_ptr(), logits.data_ptr())
            else:
                seg.identify_device(base, n, probs.data_ptr(), logits.data_ptr())
        seg.synchronize()
        if " trip" in name and not category:        # (the guard's statistics are the identity network's)
            assert seg.guard_stats() != (0, False), name
        for what, t in (("probs", probs), ("logits", logits)):
            b = t[:n].cpu().numpy().tobytes()
            index.append({"case": name, "what": what, "offset": blob.tell(), "bytes": len(b), "guard": None if category else list(seg.guard_stats())})
            blob.write(b)

    for (W, H, CH) in ((80, 80, 1), (80, 80, 3), (64, 64, 1), (100, 60, 1), (120, 16, 1)):
        st = weights.synthetic_state(CLASSES, 31, CH, W, H)
        for geom in (GEOMS if (W, CH) == (80, 1) else (0, 1 << 29) if W == 80 else (0,)):
            os.environ["TREXHIP_CONV_GEOM"] = str(geom)
            for trip in (False, True):
                seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
                seg.load_weights(weights.pack_blob(out_of_range(st) if trip else st, CLASSES, CH, W, H))
                tag = f"{W}x{H}x{CH} geom={geom}"
                if trip:        # one guard-tripping case per chain, aligned and unaligned
                    for aligned in (True, False):
                        run(seg, f"{tag} trip aligned={aligned}", real[CH] if W == 80 else pool, 5, W * H * CH, capi.CNN_FP16X3, aligned)
                else:
                    for mode in MODES:
                        if mode != capi.CNN_FP16X3 and geom != 0:      # the geometry word only matters to FP16X3
                            continue
                        for n in (COUNTS if W in (80, 64) else (33,)):
                            for aligned in (True, False):
                                run(seg, f"{tag} mode={mode} n={n} aligned={aligned}", pool, n, W * H * CH, mode, aligned)
                    if geom == 0 and (W, CH) == (80, 1):
                        run(seg, f"{tag} default n=12800", pool, 12800, W * H * CH, capi.CNN_FP16X3, True)
                seg.close()
    os.environ["TREXHIP_CONV_GEOM"] = "0"
    for (arch, W, H, CH) in ARCH_CASES:       # shapes of tests/cnn_arch_edge_cases.py and tests/category_cases.py, 33 crops each
        cat = arch == "category"
        st = weights.synthetic_category_state(CLASSES, 31, CH, W, H) if cat else weights.synthetic_state(CLASSES, 31, CH, W, H, arch=arch)
        for trip in (False, True):
            seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
            w = arch_out_of_range(st, cat) if trip else st
            if cat:
                seg.load_category_weights(weights.pack_category_blob(w, CLASSES, CH, W, H))
            else:
                seg.load_weights(weights.pack_blob(w, CLASSES, CH, W, H, arch=arch))
            for mode in ((capi.CNN_FP16X3,) if trip else MODES):
                run(seg, f"{arch} {W}x{H}x{CH} mode={mode}{' trip' if trip else ''}", pool, 33, W * H * CH, mode, True, category=cat)
            seg.close()
    blob.close()
    with open(out_path + ".json", "w") as f:
        json.dump(index, f, indent=0)
    print(f"{len(index) // 2} cases, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
