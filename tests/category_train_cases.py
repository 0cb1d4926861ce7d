"""The cases of the category network's training step (ChainTrainer in trex_amd/csrc/train_arch.hip): the smallest shapes at which each path of the 3-tap chain can go
wrong.  A plain table plus the input recipe, shared by test_category_train_ref.py (the float64 margin of the float32 restatement, on the CPU) and
test_train_category_gpu.py (the device against float64).

A case is ((W, H, channels, n, categories), seed, why).

Inputs are train_arch_cases.textured: texture on every pixel, no constant background.  The weights are weights.synthetic_category_state (a third of the
BatchNorm2d scales negative: the BatchNorm stands in front of the pool, nothing may be folded across it; the convolution weights are random, so no
kernel is symmetric and an unflipped data gradient shows) with running statistics away from 0 and 1.  The masks are drawn at 0.25 per element.

The bars are the project's own (train_arch_cases.py): gradients within GRAD_RTOL = 2e-4 of max|g64| per tensor; loss within 5e-5 relative; running
statistics within 1e-4; parameters after three steps at LR = 1e-5 within 1e-4; `correct` equal.  A convolution bias stands in front of a BatchNorm: its
true gradient is 0 and it is held to 1e-4 max(1, max|g64 of the matching weight|).

The seeds were chosen on the CPU, never after a device run: the first of seed0, seed0 + 1, ... (seed0 = 3000 + 7 W + H) at which the float32
restatement stays within a fifth of every bar of the float64 one -- test_category_train_ref.py checks that they do."""
import functools
import numpy as np
import torch

from trex_amd import weights
import category_train_ref as ref
from train_arch_cases import textured

GRAD_RTOL = 2e-4
LR = 1e-5
ZERO_GRADIENT = {"conv1.bias": "conv1.weight", "conv2.bias": "conv2.weight", "conv3.bias": "conv3.weight"}

CASES = [
    ((8, 8, 1, 3, 5), 3064, "one position in front of fc1; block 3's convolution plane is 2 x 2"),
    ((9, 8, 3, 4, 5), 3071, "a column dropped by block 1's pool, which still enters BatchNorm's statistics, dz, and both gradients; three channels"),
    ((21, 13, 3, 5, 70), 3160, "odd planes at two levels on both axes (21 -> 10 -> 5 -> 2, 13 -> 6 -> 3 -> 1); 70 categories"),
    ((13, 21, 1, 4, 7), 3112, "the transpose: a swapped W / H anywhere"),
    ((24, 16, 1, 1, 4), 3184, "n = 1 trains: every BatchNorm sees at least the 6 x 4 pixels of block 3's plane"),
    ((80, 80, 1, 3, 7), 3640, "3 x 3 conv2 tiles with origins past 0; the reference's size"),
    ((100, 60, 3, 3, 7), 3760, "ragged tiles in x and y, a second k_tany_wgrad1 strip and a ragged band (60 = 7 x 8 + 4); three channels"),
    ((14, 100, 1, 5, 7), 3198, "4-wide tiles; weight-gradient shares that straddle crops"),
    ((100, 14, 1, 3, 7), 3714, "the 16-wide tile"),
]


def shape_id(shape):
    W, H, ch, n, categories = shape
    return f"{W}x{H}x{ch}-n{n}-c{categories}"


def case_id(case):
    return shape_id(case[0])


def find(W, H):
    (case,) = [c for c in CASES if c[0][:2] == (W, H)]
    return case


def tensors(case):
    W, H, ch, n, categories = case[0]
    return weights.category_shapes(categories, ch, W, H)


def inputs(case, s=0, n=None):
    """the batch of step s: x float32 NHWC in [0, 255] with texture on every pixel, y, the element-wise keep masks at 0.25"""
    (W, H, ch, n0, categories), seed, _ = case
    n = n or n0
    seed = seed + 100 * s
    y = np.random.default_rng(seed + 1).integers(0, categories, n).astype(np.int32)
    return textured(n, seed, ch, W, H), y, ref.draw_masks(n, W, H, seed + 2)


def crops(case, n, seed):
    (W, H, ch, _, _), _, _ = case
    return textured(n, seed, ch, W, H).astype(np.uint8)


def initial_state(case):
    (W, H, ch, n, categories), seed, _ = case
    st = weights.synthetic_category_state(categories, seed, channels=ch, width=W, height=H)
    rng = np.random.default_rng(seed + 5)
    for k in st:                                  # running statistics that are not the initial 0 and 1: a step's update of them is then visible
        if k.endswith("running_mean"):
            st[k] = rng.uniform(-0.2, 0.2, st[k].shape).astype(np.float32)
        if k.endswith("running_var"):
            st[k] = rng.uniform(0.5, 2.0, st[k].shape).astype(np.float32)
    return st


@functools.lru_cache(maxsize=None)
def restatements(case):
    """the first step by the CPU restatement, computed once per case and left unchanged:
    -> {torch.float32: (loss, correct, grads, running statistics), torch.float64: the same}"""
    x, y, masks = inputs(case)
    state = initial_state(case)
    return {dt: ref.forward_backward(state, x, y, masks, dtype=dt, threads=16) for dt in (torch.float32, torch.float64)}


def gradient_error(k, g, g64):
    """-> (error, bar) of one gradient tensor against float64"""
    if k in ZERO_GRADIENT:
        return float(np.abs(g[k]).max()), 1e-4 * max(1.0, float(np.abs(g64[ZERO_GRADIENT[k]]).max()))
    return float(np.abs(g[k] - g64[k]).max()), GRAD_RTOL * float(np.abs(g64[k]).max())


def margins(case):
    """the float32 restatement's distance from the float64 one as fractions of the bars: {what: fraction}"""
    both = restatements(case)
    l32, c32, g32, s32 = both[torch.float32]
    l64, c64, g64, s64 = both[torch.float64]
    out = {"loss": abs(l32 - l64) / (5e-5 * max(1.0, abs(l64))), "correct": 0.0 if c32 == c64 else float("inf")}
    for k in g64:
        err, bar = gradient_error(k, g32, g64)
        out[k] = err / bar
    for k in s64:
        out[k] = float(np.abs(s32[k] - s64[k]).max()) / (1e-4 * max(1.0, float(np.abs(s64[k]).max())))
    return out
