"""The cases of the category network (trexhip_categorize_device): the smallest shapes at which each path of its chain can go wrong.  A plain table
plus the recipe of weights and inputs, shared by make_category_fixture.py (the reference's vectors), test_category_ref.py (what each case reaches
and the float64 margin of the float32 restatement, on the CPU) and test_categorize_gpu.py (the device).

A case is ((W, H, channels, categories), seed, why).

Inputs are textured to the crop's edge (train_arch_cases.textured), so the border taps -- where the padding of the normalised image matters -- carry
weight.  The seeds were chosen on the CPU, never after a device run: the first of seed0, seed0 + 1, ... (seed0 = 3000 + 7 W + H) at which no crop of
n = 1 or 37 has a float64 top-two logit gap below 2 x 8 x e32 (e32 = the float32 restatement's distance from float64); test_category_ref.py checks it.
"""
import functools
import os
import numpy as np

from trex_amd import weights
from train_arch_cases import textured

BATCHES = (1, 37)
LOGIT_FACTOR = 8            # the device may be this many times the float32 restatement's own distance from float64 (test_cnn_trained_gpu.py)
UNDECIDED_CAP = 0.01        # the project's cap on crops a test may leave undecided; the chosen inputs stay at 0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "category.npz")

CASES = [
    ((8, 8, 1, 1024), 3064, "fc1 sees one position; 1024 categories: every repetition of the head and of the label's scan"),
    ((9, 8, 3, 2), 3071, "a dropped column in block 1; three channels"),
    ((21, 13, 3, 70), 3160, "odd planes at two levels on both axes (21 -> 10 -> 5 -> 2, 13 -> 6 -> 3 -> 1); a second 64-lane repetition of the head"),
    ((13, 21, 1, 3), 3112, "the transpose: a swapped W / H anywhere"),
    ((80, 80, 1, 5), 3640, "the default individual_image_size: 3 x 3 tiles in conv2 (origins past 0 on both axes), 4-wide tiles in conv3"),
    ((100, 60, 3, 3), 3760, "seven 4-wide tiles in a row in conv2 (ragged in x and y), two tiles in conv3, two rows of first-layer tiles; three channels"),
    ((14, 100, 1, 5), 3198, "the 4-wide tile in conv2 (7 x 50 windows)"),
    ((100, 14, 1, 2), 3714, "the 16-wide tile in conv2 (50 x 7 windows)"),
]


def case_id(case):
    W, H, ch, cats = case[0]
    return f"{W}x{H}x{ch}-c{cats}"


def crops(case, n):
    (W, H, ch, _), seed, _ = case
    return textured(n, seed + 1000 + n, ch, W, H).astype(np.uint8)


def calibration_crops(case):
    (W, H, ch, _), seed, _ = case
    return textured(64, seed + 1, ch, W, H).astype(np.uint8)


def raw_state(case):
    (W, H, ch, cats), seed, _ = case
    return weights.synthetic_category_state(cats, seed, ch, W, H)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def state(case):
    """the recipe's weights with the running statistics the reference model calibrated (stored in the fixture)"""
    st = raw_state(case)
    fx = fixture()
    for k in st:
        if "running_" in k:
            st[k] = fx[f"case/{case_id(case)}/stat/{k}"]
    return st


def blob(case):
    (W, H, ch, cats), _, _ = case
    return weights.pack_category_blob(state(case), cats, ch, W, H)
