"""The cases of the v100 / v110 training step (trex_amd/csrc/train_arch.hip): the smallest shapes at which each new path can go wrong.  A plain
table plus the input recipe, shared by test_train_arch_ref.py (what each case reaches, by arithmetic; the float64 margin of the float32
restatement; on the CPU) and test_train_arch_gpu.py (the device against float64).  Every case runs for both versions.

A case is ((W, H, channels, n, classes), seed, why).

Inputs carry texture on every pixel: uniform noise in [8, 248) on a per-crop ramp, no constant background.  On weights.synthetic_crops' black
background conv2 and conv3 see constant neighbourhoods, and v110's pool on raw outputs meets near-ties whose arg-max differs between float32 and
float64 (the reference's own float32 was 2.9e-2 from its float64 on conv3.weight at 80 x 80 that way).  v110 cases use n >= 3: BatchNorm over two
values is ill-conditioned (the float32 reference is 2.6e-4 to 3.3e-4 from float64 at n = 2).

The seeds were chosen on the CPU, never after a device run: the first of seed0, seed0 + 1, ... (seed0 = 2000 + 7 W + H) at which the float32
restatement of both versions stays within a fifth of every bar of the float64 one -- test_train_arch_ref.py checks that they do."""
import functools
import numpy as np
import torch

from trex_amd import weights
import train_arch_ref as ref

ARCHS = ("v100", "v110")
GRAD_RTOL = 2e-4
LR = 1e-5      # of the chained steps: Adam moves an element by up to lr per step whatever its gradient's size, in an arbitrary direction where the
               # gradient is rounding noise, so two correct chains part by up to 2 lr per step: 3 steps x 2e-5 = 6e-5 stays inside the parameters' 1e-4

CASES = [
    ((8, 8, 1, 3, 5), 2065, "the pooled plane in front of fc1 is 1 x 1 and block 3's BatchNorm2d count is n"),
    ((9, 8, 3, 4, 5), 2071, "an odd conv1 plane: one column dropped by the floor pool of block 1; three channels"),
    ((21, 13, 3, 5, 100), 2160, "odd planes at blocks 1 and 3 on both axes (21 -> 10 -> 5 -> 2, 13 -> 6 -> 3 -> 1); 100 classes"),
    ((13, 21, 1, 4, 7), 2112, "the transpose: a swapped W / H anywhere"),
    ((44, 28, 1, 3, 7), 2336, "an odd plane at block 3 only (11 x 7)"),
    ((80, 80, 1, 3, 7), 2640, "the size that must not take the tuned V118_3 kernels"),
    ((100, 60, 3, 3, 7), 2761, "several convolution tiles in both layers (375 and 104 windows), a second k_tany_wgrad1 strip and a ragged band (60 = 7 x 8 + 4); three channels"),
    ((14, 100, 1, 5, 7), 2198, "two conv2 tiles 4 windows wide; ragged weight-gradient shares in both layers (250 rows in 84 x 3, 125 in 42 x 3) that straddle crops"),
]


def shape_id(shape):
    W, H, ch, n, classes = shape
    return f"{W}x{H}x{ch}-n{n}-c{classes}"


def case_id(case):
    return shape_id(case[0])


def find(W, H):
    (case,) = [c for c in CASES if c[0][:2] == (W, H)]
    return case


def levels(W, H):
    """the planes of z1, z2, z3 and of fc1's input, by successive floors"""
    out = [(W, H)]
    for _ in range(3):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def textured(n, seed, ch, W, H):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    x = rng.uniform(8.0, 248.0, (n, H, W, ch))
    ramp = (xx[None, :, :, None] * rng.uniform(-1, 1, (n, 1, 1, 1)) + yy[None, :, :, None] * rng.uniform(-1, 1, (n, 1, 1, 1))) * (60.0 / max(W, H))
    return np.ascontiguousarray(np.clip(x + ramp, 0.0, 255.0), np.float32)


def inputs(case, arch, s=0, n=None):
    """the batch of step s: x float32 NHWC in [0, 255] with texture on every pixel, y, the keep masks at the architecture's rates"""
    (W, H, ch, n0, classes), seed, _ = case
    n = n or n0
    seed = seed + 100 * s
    y = np.random.default_rng(seed + 1).integers(0, classes, n).astype(np.int32)
    return textured(n, seed, ch, W, H), y, ref.draw_masks(arch, n, seed + 2)


def crops(case, n, seed):
    (W, H, ch, _, _), _, _ = case
    return textured(n, seed, ch, W, H).astype(np.uint8)


def initial_state(case, arch):
    (W, H, ch, n, classes), seed, _ = case
    st = weights.synthetic_state(classes, seed, channels=ch, width=W, height=H, arch=arch)
    rng = np.random.default_rng(seed + 5)
    for k in st:                                  # running statistics that are not the initial 0 and 1: a step's update of them is then visible
        if k.endswith("running_mean"):
            st[k] = rng.uniform(-0.2, 0.2, st[k].shape).astype(np.float32)
        if k.endswith("running_var"):
            st[k] = rng.uniform(0.5, 2.0, st[k].shape).astype(np.float32)
        if k in ("bn1.weight", "bn2.weight", "bn3.weight"):        # a third of the BatchNorm2d scales negative: nothing may be folded across v110's pool
            st[k] = (st[k] * np.where(rng.random(st[k].shape) < 1 / 3, -1.0, 1.0)).astype(np.float32)
    return st


@functools.lru_cache(maxsize=None)
def restatements(case, arch):
    """the first step by the CPU restatement, computed once per case and version and left unchanged:
    -> {torch.float32: (loss, correct, grads, running statistics), torch.float64: the same}"""
    x, y, masks = inputs(case, arch)
    state = initial_state(case, arch)
    return {dt: ref.forward_backward(arch, state, x, y, masks, dtype=dt, threads=16) for dt in (torch.float32, torch.float64)}


def margins(case, arch):
    """the float32 restatement's distance from the float64 one as fractions of the bars: {what: fraction}"""
    both = restatements(case, arch)
    l32, c32, g32, s32 = both[torch.float32]
    l64, c64, g64, s64 = both[torch.float64]
    out = {"loss": abs(l32 - l64) / (5e-5 * max(1.0, abs(l64))), "correct": 0.0 if c32 == c64 else float("inf")}
    zero = ref.zero_gradient(arch)
    for k in g64:
        if k in zero:
            out[k] = float(np.abs(g32[k]).max()) / (1e-4 * max(1.0, float(np.abs(g64[zero[k]]).max())))
        else:
            out[k] = float(np.abs(g32[k] - g64[k]).max()) / (GRAD_RTOL * float(np.abs(g64[k]).max()))
    for k in s64:
        out[k] = float(np.abs(s32[k] - s64[k]).max()) / (1e-4 * max(1.0, float(np.abs(s64[k]).max())))
    return out
