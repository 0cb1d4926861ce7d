"""The forward passes of TRex's v100, v110, v119 and v200 identity networks, restated from the layer table
(trex_amd.weights.ARCH_LAYERS) with torch.nn.functional, in float32 or float64: the CPU reference of the architecture chains
(cnn_arch.hip).  Convolutions are 'same', pools floor, inputs are raw float(byte), dropout is identity, BatchNorm is eval-mode
with eps 1e-5.  test_cnn_arch_ref.py holds this restatement to the reference's own vectors (tests/golden/cnn_arch.npz)."""
import os
import numpy as np
import torch
import torch.nn.functional as F
from trex_amd import weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnn_arch.npz")
ARCHS = ("v100", "v110", "v119", "v200")
# (W, H, CH) per architecture; 8 classes; the seed is 500 + 10 * architecture id + case index
SIZES = {"v100": [(8, 8, 1), (52, 52, 3), (100, 60, 1), (80, 80, 1)],
         "v110": [(8, 8, 1), (52, 52, 3), (100, 60, 1), (80, 80, 1)],
         "v119": [(16, 16, 1), (52, 52, 3), (100, 60, 1), (80, 80, 1)],
         "v200": [(27, 27, 1), (52, 52, 3), (100, 60, 1), (80, 80, 1)]}
CLASSES = 8
CASES = [(a, w, h, ch, CLASSES, 500 + 10 * weights.ARCH_IDS[a] + i) for a in ARCHS for i, (w, h, ch) in enumerate(SIZES[a])]
BATCHES = (1, 37)


def case_id(case):
    return f"{case[0]}-{case[1]}x{case[2]}x{case[3]}"


def _bn(x, t, name):
    return F.batch_norm(x, t[name + ".running_mean"], t[name + ".running_var"], t[name + ".weight"], t[name + ".bias"], training=False, eps=1e-5)


# V118_3 in the same table form (tools/time_identify_versions.py times all five beside torch): BatchNorm in front of the pool, LayerNorm behind fc1
V118_3 = dict(convs=[(16, 5), (64, 5), (128, 5)], bn2d=True, hidden=100, bn1d=None)


def forward_tensors(t, x, arch):
    """t: state dict of tensors, x: NCHW tensor of the same dtype and device -> logits; the layer table walked with torch.nn.functional"""
    arch = weights.arch_name(arch)
    L = V118_3 if arch == "v118_3" else weights.ARCH_LAYERS[arch]
    for i, (co, k) in enumerate(L["convs"], 1):
        x = F.conv2d(x, t[f"conv{i}.weight"], t[f"conv{i}.bias"], padding=k // 2)
        if arch == "v100":
            x = F.max_pool2d(F.relu(x), 2)
        elif arch == "v110":                   # the BatchNorm sits behind the pool
            x = F.relu(_bn(F.max_pool2d(x, 2), t, f"bn{i}"))
        elif arch in ("v119", "v118_3"):
            x = F.max_pool2d(F.relu(_bn(x, t, f"bn{i}")), 2)
        else:                                  # v200: pool3 behind conv2, conv4 and conv5
            x = F.relu(_bn(x, t, f"bn{i}"))
            if i in (2, 4, 5):
                x = F.max_pool2d(x, 3)
    x = x.mean((2, 3)) if arch == "v200" else x.reshape(x.shape[0], -1)
    x = F.linear(x, t["fc1.weight"], t["fc1.bias"])
    if arch == "v118_3":
        x = F.layer_norm(x, (100,), t["bn4.weight"], t["bn4.bias"], eps=1e-5)
    elif L["bn1d"]:
        x = _bn(x, t, L["bn1d"])
    return F.linear(F.relu(x), t["fc2.weight"], t["fc2.bias"])


def forward(st, crops, arch, dtype=torch.float64, threads=8):
    """st: state dict of numpy arrays; crops: uint8 [n][H][W][CH] -> (probs, logits) as numpy arrays of `dtype`"""
    torch.set_num_threads(threads)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in st.items()}
    with torch.no_grad():
        logits = forward_tensors(t, torch.from_numpy(np.ascontiguousarray(crops)).to(dtype).permute(0, 3, 1, 2), arch)
        probs = F.softmax(logits, 1)
    return probs.numpy(), logits.numpy()


_Z = None


def load_case(case):
    """-> (state with the fixture's running statistics, {n: (probs, logits)} of the reference, {n: crops})"""
    global _Z
    if _Z is None:
        _Z = np.load(GOLDEN)
    arch, w, h, ch, classes, seed = case
    st = weights.synthetic_state(classes, seed, ch, w, h, arch=arch)
    pre = f"case/{case_id(case)}/"
    for k in st:
        if "running_" in k:
            st[k] = _Z[pre + "stat/" + k]
    want = {n: (_Z[pre + f"probs/{n}"], _Z[pre + f"logits/{n}"]) for n in BATCHES}
    crops = {n: weights.synthetic_crops(n, seed + 1000 + n, ch, w, h) for n in BATCHES}
    return st, want, crops
