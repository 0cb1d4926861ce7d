"""The edge cases of the architecture chains (cnn_arch.hip): the smallest shapes at which every tile shape, channel block, tap count and pool of
k_arch_conv, the odd sizes of k_arch_conv1, k_pool3 and k_gap over more than one position, and every repetition pattern of k_arch_head run.
A plain table, shared by test_cnn_arch_edge_plan.py (what each case reaches, from the plan, on the CPU) and test_cnn_arch_edges_gpu.py (float64).

A case is (arch, W, H, CH, classes, n, seed, why).  n * classes >= 512 throughout: e32, the float32 restatement's own error, is a maximum
over at least that many logits.  In `why`, a layer behind the first is TX/taps/pool/COB over wy x wx windows of 2 x 2 conv pixels
(pool 2: the pooled output; no pool: ceil(Hi / 2) x ceil(Wi / 2)); a tile is TX windows wide and 64 / TX high."""
import numpy as np
from trex_amd import weights

CASES = [
    # ---- the 16-wide tile (wide, short crops) ----
    ("v100", 69, 13, 1, 100, 31, 900, "L1 16/5/2/64 over 3x17: two tiles, ragged in x and y; first layer odd W and H under its pool"),
    ("v110", 69, 13, 3, 65, 33, 901, "as above with the affine behind the pool and 3 channels; 65 classes: one lane of a second repetition"),
    ("v100", 75, 19, 1, 63, 32, 902, "L1 16/5/2/64 over 4x18, L2 16/5/2/128 over 2x9 (ragged in y); 63 classes: a partial only repetition"),
    ("v119", 75, 19, 1, 257, 2, 903, "L1 16/5/2/128 over 4x18 (CI 256), L2 16/5/2/32 over 2x9: one tile, ragged in x and y; 257 classes"),
    ("v119", 137, 27, 1, 1024, 1, 904, "L2 16/5/2/32 over 3x17: two tiles; L1 8/5/2/128 over 6x34; 1024 classes, one crop"),
    ("v200", 93, 54, 1, 64, 8, 905, "L1 16/3/0/128 over 27x47: 3 x 7 tiles; L2, L3 16/3/0/128 over 9x16 with 2 and 4 channel blocks; k_pool3 on 54x93 and 18x31"),
    ("v200", 95, 55, 3, 1024, 1, 906, "as above with 3 channels and odd W and H in the unpooled first layer; k_pool3 on 55x95; 1024 classes"),
    # ---- the 4-wide tile (tall, narrow crops): the transposes ----
    ("v100", 13, 69, 1, 100, 6, 907, "L1 4/5/2/64 over 17x3: two tiles, ragged in x and y"),
    ("v100", 19, 75, 1, 64, 8, 908, "L1 4/5/2/64 over 18x4, L2 4/5/2/128 over 9x2; 64 classes: exactly one repetition"),
    ("v119", 19, 75, 1, 100, 6, 909, "L1 4/5/2/128 over 18x4, L2 4/5/2/32 over 9x2"),
    ("v200", 54, 93, 1, 100, 6, 910, "L1 4/3/0/128 over 47x27: 7 x 3 tiles; L2, L3 4/3/0/128 over 16x9; last layer leaves 3x2: k_gap over 6 positions"),
    # ---- the first layer at and one past its 32-pixel tile ----
    ("v100", 32, 32, 1, 64, 31, 911, "first layer: exactly one 32 x 32 tile"),
    ("v110", 33, 33, 1, 100, 33, 912, "first layer: one pixel past the tile, dropped by the pool's floor; 33 crops: a second row block of fc1"),
    ("v100", 65, 33, 3, 257, 2, 913, "first layer: 2 tiles in x (65 / 2 = 32 windows) and the odd column; last layer leaves 4x8: the fc1 reorder"),
    # ---- the 8x8 tile with ragged edges, P > 1 and P = 1 ----
    ("v110", 37, 35, 1, 64, 32, 914, "L1 8/5/2/64 over 8x9: ragged in x; last layer leaves 4x4"),
    ("v119", 45, 43, 3, 100, 6, 915, "L1 4/5/2/128 over 10x11: 3 tiles; L2 8/5/2/32 over 5x5, L3 8/5/2/128 over 2x2: ragged in x and y"),
    ("v200", 55, 29, 1, 100, 6, 916, "L1 4/3/0/128 over 15x28: 7 tiles; L2, L3 8/3/0/128 over 5x9: ragged in x and y; k_gap over 1x2"),
    ("v200", 27, 27, 1, 2, 257, 917, "the minimum: every pool leaves one pixel; 2 classes; 257 crops"),
    ("v119", 16, 16, 1, 65, 33, 918, "the minimum: the last layer leaves 1x1"),
    # ---- the head's repetitions on the smallest shape ----
    ("v100", 8, 8, 1, 1, 512, 919, "1 class: the softmax is exactly 1.0"),
    ("v100", 8, 8, 1, 1024, 1, 920, "1024 classes: all 16 repetitions, one crop"),
    ("v110", 8, 8, 3, 257, 33, 921, "257 classes: four full repetitions and one lane of a fifth; BatchNorm1d in front of them"),
]

MIN_LOGITS = 512


def case_id(case):
    return f"{case[0]}-{case[1]}x{case[2]}x{case[3]}-c{case[4]}-n{case[5]}"


def make(case):
    """-> (state, crops) of a case.  weights.synthetic_crops draws one ellipse in the middle of the frame, which leaves the borders of a wide
    or tall crop black (93x54: 8 % filled): every window at a ragged edge would see the same constant background, and a wrong column there would
    change nothing.  So the later half of a case's crops (n = 1: the crop) gets texture on every background pixel as well."""
    arch, w, h, ch, classes, n, seed, _ = case
    st = weights.synthetic_state(classes, seed, ch, w, h, arch=arch)
    crops = weights.synthetic_crops(n, seed + 1000, ch, w, h)
    rng = np.random.default_rng(seed + 2000)
    late = crops[n // 2:]
    late[late == 0] = rng.integers(1, 256, late.shape, dtype=np.uint8)[late == 0]
    return st, crops
