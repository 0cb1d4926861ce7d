"""What the cases of train_tile_cases.py reach, shown on the CPU from the geometry printer (tests/cpp/test_train_geom.cpp, the plain build), and
the condition under which test_train_tiles_gpu.py may hold the device to float64: the float32 restatement of every case agrees with its float64
self five times closer than the gradient bar (GRAD_RTOL / 5, the margin test_train_sizes_gpu.py states for its own shapes), the losses to 1e-5.
Measured with the table's seeds: worst gradient ratio 1.26e-5 max|g64| (80 x 72, conv2.weight), 1.08e-5 at 100 x 60, at most 3.5e-6 at the other
four; the losses agree to 2.1e-6.  A case that misses the condition gets another seed, never a wider bar: a miss would be a max-pool near-tie
that the two precisions resolve differently."""
import os
import subprocess
import numpy as np
import pytest
import torch

from oracle import cnn_train_oracle as tro
from test_train_geom import HIPCC, ROOT, geom
from train_tile_cases import CASES, CONV_BIAS, GEOMETRY_KEYS, GRAD_RTOL, SIZES_SHAPES, case_id, inputs, restatements


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("train_tile_cases") / "test_train_geom_plain")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_train_geom.cpp"), "-o", path])
    return path


def reached(exe, shape):
    """the geometry of a shape at its own n, as numbers: conv2 / conv3 -> (TX, tiles per row, tile rows), wgrad1 -> (strips, workgroups),
    wgrad2 / wgrad3 -> (per, shares, rows of the batch, rows of a crop)"""
    W, H, ch, n, _ = shape
    g = geom(exe, W, H, ch, n)
    out = {"W": W, "H": H}
    for k in ("conv2", "conv3"):
        tx, per_row, tiles = (int(v) for v in g[k].split(","))
        assert tiles % per_row == 0
        out[k] = (tx, per_row, tiles // per_row)
    out["wgrad1"] = tuple(int(v) for v in g["wgrad1"].split(","))
    for k, plane in (("wgrad2", "z2"), ("wgrad3", "z3")):
        _, per, shares = (int(v) for v in g[k].split(","))
        h = int(g[plane].split("x")[1])
        out[k] = (per, shares, n * h, h)
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_case_has_the_geometry_the_table_states(exe, case):
    (W, H, ch, n, _), want, _ = case
    g = geom(exe, W, H, ch, n)
    assert set(want) == set(GEOMETRY_KEYS)
    assert {k: g[k] for k in GEOMETRY_KEYS} == want, g


def test_the_table_reaches_every_tile_shape_strip_and_share(exe):
    r = [reached(exe, c[0]) for c in CASES]
    for layer in ("conv2", "conv3"):
        assert {g[layer][0] for g in r} == {4, 8, 16}, layer                                 # each of the three tile shapes, in each layer
    assert any(g[layer][1] > 1 and g[layer][2] > 1 for g in r for layer in ("conv2", "conv3"))  # a grid of tiles: x0 > 0 and y0 > 0 at once
    assert any(g[layer][0] == 8 and g[layer][1] > 1 and g[layer][2] > 1 for g in r for layer in ("conv2", "conv3"))   # ... of 8 x 8 tiles
    assert any(g["wgrad1"][0] > 1 and g["W"] % 64 for g in r)                               # a second strip, and a ragged last one
    for layer in ("wgrad2", "wgrad3"):
        assert any(per * shares > rows for per, shares, rows, _ in (g[layer] for g in r)), layer                 # a last share that the clamp cuts
        assert any(per * shares == rows and per > 1 for per, shares, rows, _ in (g[layer] for g in r)), layer    # and one it does not
    assert any(per > 1 and h % per for layer in ("wgrad2", "wgrad3") for per, _, _, h in (g[layer] for g in r))  # a share across two crops
    assert any(g["W"] == 256 for g in r) and any(g["H"] == 256 for g in r)                   # both axes at their maximum


def test_the_four_shapes_of_test_train_sizes_gpu_reach_none_of_it(exe):
    """for the record: when this fails because that file grew, the table above can shrink"""
    r = [reached(exe, s) for s in SIZES_SHAPES]
    assert all(g[layer][0] != 4 for g in r for layer in ("conv2", "conv3"))                  # no 4-wide tile
    assert all(g["conv3"][0] != 16 for g in r)                                               # no 16-wide tile in conv3
    assert all(g[layer][1] == 1 for g in r for layer in ("conv2", "conv3"))                  # one tile per row: x0 = 0 everywhere, no grid of tiles
    assert all(g["wgrad1"][0] == 1 for g in r)                                               # one strip
    assert all(per * shares == rows for g in r for per, shares, rows, _ in (g["wgrad2"], g["wgrad3"]))   # no ragged share
    assert all(max(s[:2]) < 256 for s in SIZES_SHAPES)


def crosses(x, axis, boundaries):
    """does the blob of some crop of x [n][H][W][ch] lie on both sides of one of the boundaries along the axis (1: rows, 2: columns)?"""
    for crop in x:
        at = np.flatnonzero((crop > 0).any(axis=tuple(a for a in (0, 1, 2) if a != axis - 1)))
        if any(at[0] < b <= at[-1] for b in boundaries):
            return True
    return False


def test_the_blobs_lie_across_the_boundaries_that_the_cases_are_there_for(exe):
    """The recipe's crops are one blob on black (weights.synthetic_crops), and a wide or tall crop is mostly background: 256 x 8 is black outside
    columns 107..149, and the second strip of 80 x 72 is all black, so conv1's weight gradient there is 0 whatever the kernel reads.  The forward
    tiles and k_tany_wgrad1 can show a wrong origin or halo only where the input has texture (the data gradients and k_tany_wgrad see dz, which
    differs everywhere).  So: in every case with more than one conv2 tile along an axis a blob lies across a tile boundary of that axis (a tile is
    4 TX input pixels wide and 4 x 64 / TX high), and a blob lies across a strip boundary (64 columns) in a case whose last strip is ragged and in
    one whose strips are full"""
    ragged_strip = full_strips = False
    for case in CASES:
        shape = case[0]
        W, H = shape[:2]
        x = inputs(*shape, 0)[0]
        tx, per_row, tile_rows = reached(exe, shape)["conv2"]
        if per_row > 1:
            assert crosses(x, 2, range(4 * tx, W, 4 * tx)), case_id(case)
        if tile_rows > 1:
            assert crosses(x, 1, range(4 * (64 // tx), H, 4 * (64 // tx))), case_id(case)
        if W > 64 and crosses(x, 2, range(64, W, 64)):
            ragged_strip, full_strips = ragged_strip or W % 64 != 0, full_strips or W % 64 == 0
    assert ragged_strip and full_strips


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_float32_restatement_is_five_times_inside_the_bar_of_float64(case):
    both = restatements(case[0])
    loss32, correct32, g32, stats32 = both[torch.float32]
    loss64, correct64, g64, stats64 = both[torch.float64]
    worst = 0.0
    for k in tro.TRAINABLE:
        assert g64[k].dtype == np.float64 and g32[k].dtype == np.float32
        if k in CONV_BIAS:                       # in front of a BatchNorm: the true gradient is 0, both restatements hold rounding noise
            continue
        ratio = float(np.abs(g32[k] - g64[k]).max()) / float(np.abs(g64[k]).max())
        worst = max(worst, ratio)
        print(f"{case_id(case)} {k}: max|g32 - g64| = {ratio:.3g} max|g64|")
        assert ratio <= GRAD_RTOL / 5, (k, ratio)
    print(f"{case_id(case)}: worst {worst:.3g}, |loss32 - loss64| = {abs(loss32 - loss64):.3g}, correct {correct32} / {correct64}")
    assert abs(loss32 - loss64) <= 1e-5
    assert correct32 == correct64
    for k in tro.BUFFERS:
        assert np.abs(stats32[k] - stats64[k]).max() <= 2e-5 * max(1.0, float(np.abs(stats64[k]).max())), k      # a fifth of the device's bar
