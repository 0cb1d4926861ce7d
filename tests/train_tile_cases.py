"""The tile-shape and share cases of the any-size training step (train_any.hip): the smallest batches at which every tile shape of k_tany_conv, a
tile with x0 > 0, a second strip of k_tany_wgrad1, a ragged last share of k_tany_wgrad and both axes at 256 run.  A plain table plus the input
recipe, shared by test_train_tile_cases.py (what each case reaches, from the geometry printer, on the CPU; the float64 margin of the
restatement) and test_train_tiles_gpu.py (the device against float64).

A case is ((W, H, channels, n, classes), geometry, why).  The geometry is what tests/cpp/test_train_geom.cpp prints at the case's own n:
   conv2, conv3    TX, tiles per row, tiles     (a tile is TX pool windows wide and 64 / TX high, over ceil(h / 2) x ceil(w / 2) windows)
   wgrad1          strips per band, workgroups per crop     (8 rows x 64 columns each)
   wgrad2, wgrad3  types, per, shares           (the n h rows of the batch in runs of `per`)
The inputs are test_train_sizes_gpu.py's, from its own helpers: weights.synthetic_state(classes, seed, channels, W, H), train_batch and draw_masks
with seed 1000 + 7 W + H (+ 100 per further step), LR = 1e-3."""
import functools
import torch
from trex_amd import weights
from oracle import cnn_train_oracle as tro
from test_train_sizes_gpu import GRAD_RTOL, LR, CONV_BIAS, SHAPES as SIZES_SHAPES, inputs      # noqa: F401  (re-exported: one recipe, not two)

CASES = [
    ((14, 100, 1, 5, 7), dict(conv2="4,1,2", conv3="4,1,1", wgrad1="1,13", wgrad2="5,3,84", wgrad3="10,3,42"),
     "4-wide tiles in both layers; conv2: 7 x 50 pixels = 4 x 25 windows, two tile rows, the second ragged, ragged in x; odd planes 7 x 50 and 3 x 25; "
     "both weight gradients end in a ragged share (250 rows in 84 x 3, 125 in 42 x 3) and their shares straddle crops (50 and 25 rows per crop)"),
    ((100, 14, 3, 15, 7), dict(conv2="16,2,2", conv3="16,1,1", wgrad1="2,4", wgrad2="5,2,53", wgrad3="10,1,45"),
     "16-wide tiles in both layers, two per row in conv2 (25 windows); two wgrad1 strips, the second 36 columns wide; three channels; a ragged "
     "wgrad2 share (105 rows in 53 x 2); per = 1 in wgrad3"),
    ((100, 60, 3, 5, 100), dict(conv2="4,7,7", conv3="8,2,2", wgrad1="2,16", wgrad2="5,2,75", wgrad3="10,2,38"),
     "seven 4-wide tiles in one row (25 x 15 windows), ragged at the bottom and the right; two 8 x 8 tiles per row in conv3 (13 x 8 windows); two strips "
     "and a ragged band (60 = 7 x 8 + 4); wgrad2 exact with per = 2 (150 rows), a ragged wgrad3 share (75 rows in 38 x 2); 84 fc1 positions, 100 classes"),
    ((80, 72, 1, 3, 5), dict(conv2="8,3,9", conv3="4,3,3", wgrad1="2,18", wgrad2="5,2,54", wgrad3="10,2,27"),
     "a 3 x 3 grid of 8 x 8 tiles, ragged on both axes (20 x 18 windows); three 4-wide tiles per row in conv3 (10 x 9 windows); W = 80 with H != 80: "
     "the generic chain; a second strip 16 columns wide (all background with these crops: what it adds to conv1's weight gradient is 0); both weight gradients exact with per = 2 (108 and 54 rows)"),
    ((8, 256, 1, 2, 5), dict(conv2="4,1,4", conv3="4,1,2", wgrad1="1,32", wgrad2="5,3,86", wgrad3="10,3,43"),
     "H at its maximum; four tile rows (2 x 64 windows); a tile 2 windows wide inside a 4-wide shape; ragged shares in both layers (256 rows in "
     "86 x 3, 128 in 43 x 3)"),
    ((256, 8, 1, 2, 5), dict(conv2="16,4,4", conv3="16,2,2", wgrad1="4,4", wgrad2="5,1,8", wgrad3="10,1,4"),
     "W at its maximum; four full strips; four 16-wide tiles per row (64 x 2 windows); a tile 2 windows high inside a 4-high shape"),
]
GEOMETRY_KEYS = ("conv2", "conv3", "wgrad1", "wgrad2", "wgrad3")


def shape_id(shape):
    W, H, ch, n, classes = shape
    return f"{W}x{H}x{ch}-n{n}-c{classes}"


def case_id(case):
    return shape_id(case[0])


def find(W, H):
    """the shape of the table's case at W x H"""
    (shape,) = [c[0] for c in CASES if c[0][:2] == (W, H)]
    return shape


def initial_state(shape):
    W, H, ch, n, classes = shape
    return weights.synthetic_state(classes, 1000 + 7 * W + H, channels=ch, width=W, height=H)


@functools.lru_cache(maxsize=None)
def restatements(shape):
    """the first step's forward and backward by the CPU restatement, computed once per case and left unchanged:
    -> {torch.float32: (loss, correct, grads, running statistics), torch.float64: the same}"""
    x, y, masks = inputs(*shape, 0)
    state = initial_state(shape)
    return {dt: tro.forward_backward(state, x, y, masks, threads=16, dtype=dt)[:4] for dt in (torch.float32, torch.float64)}
