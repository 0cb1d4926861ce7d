"""The windowed instance of the role-split conv1+conv2 kernel computes, for a crop whose blob fits 8 of a row's 10 conv2 tiles, only those
tiles of only the needed rows, and takes the rest from images of an all-zero crop (trex_amd/csrc/cnn_skipx.h); the other crops take the
full-width instance.  Every result must be, bit for bit, that of a run with the windowed form switched off (TREXHIP_CONV_GEOM bit 23), of a
run that computes every pass (bit 27) and of the two-kernel chain (bit 28).  Bit 29 forces the role-split kernel at small batches."""
import os
import numpy as np
import pytest
import torch
from trex_amd import weights
from cnn_skip_driver import blob, forward, same, state  # noqa: F401  (state: the module's fixture)

pytestmark = pytest.mark.gpu

RS, NOX, NOSKIP, TWO = 1 << 29, 1 << 29 | 1 << 23, 1 << 29 | 1 << 27, 1 << 28


def listed_passes(crops):
    """the aligned passes the row rule lists, from the crops' bytes alone: V3 row gp of a crop reads its rows 4 gp - 6 .. 4 gp + 9, a pass is 3
    consecutive V3 rows of the batch"""
    need = np.zeros(20 * len(crops), bool)
    for i, c in enumerate(crops):
        rows = np.flatnonzero(c.reshape(80, -1).any(1))
        if len(rows):
            need[20 * i:20 * i + 20] = [4 * gp + 9 >= rows[0] and 4 * gp - 6 <= rows[-1] for gp in range(20)]
    return sum(bool(need[p:p + 3].any()) for p in range(0, len(need), 3))


def check(monkeypatch, st, crops, both=False):
    """-> skipx_stats of the windowed run; its skip_stats are those of the run without the windowed form (both: -> those two as well)"""
    on, g_on, s_on = forward(monkeypatch, st, RS, crops)
    nox, g_nox, s_nox = forward(monkeypatch, st, NOX, crops)
    off, g_off, _ = forward(monkeypatch, st, NOSKIP, crops)
    two, g_two, _ = forward(monkeypatch, st, TWO, crops)
    assert g_on == g_nox == g_off == g_two == (0, False)
    assert np.all(np.isfinite(on[0][0])) and np.allclose(on[0][0].sum(1), 1.0, atol=1e-5)
    for name, other in (("bit 23", nox), ("bit 27", off), ("bit 28", two)):
        assert same(on[0], other[0]), (name, float(np.abs(on[0][1] - other[0][1]).max()), np.flatnonzero(np.any(on[0][1] != other[0][1], axis=1))[:10])
    assert s_on[0][0] == s_nox[0][0]                          # SK_LEN, SK_NPASS, SK_FILLED keep their meaning
    assert s_nox[0][1] == (0, 0, 0)                           # switched off: the new words are not written
    return (s_on[0][1], s_on[0][0], s_nox[0][0]) if both else s_on[0][1]


def test_one_pixel_in_row_r_column_c(monkeypatch, state):
    """a column rule that is off by one in either direction, or a wrong t0, drops a tile one of these 80 crops needs"""
    crops = np.zeros((80, 80, 80, 1), np.uint8)
    for r in range(80):
        crops[r, r, (37 * r + 11) % 80, 0] = 255
    # a pixel reaches 2 to 4 V3 rows and at most 3 tiles: every crop has a window and one windowed pass, no full-width pass is left
    assert check(monkeypatch, state, crops) == (80, 80, 0)


def test_blobs_touching_the_edges(monkeypatch, state):
    rng = np.random.default_rng(5)
    crops = np.zeros((8, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(0, 12), slice(0, 9), rng)            # row 0 and column 0
    blob(crops, 1, slice(68, 80), slice(71, 80), rng)         # row 79 and column 79
    blob(crops, 2, slice(0, 80), slice(0, 4), rng)            # every row, column 0: five windowed passes
    blob(crops, 3, slice(0, 80), slice(76, 80), rng)          # every row, column 79
    blob(crops, 4, slice(0, 3), slice(30, 58), rng)           # row 0, tiles 3 .. 7 -> t0 = 2
    blob(crops, 5, slice(77, 80), slice(14, 66), rng)         # row 79, tiles 1 .. 8 (exactly 8) -> t0 = 1
    blob(crops, 6, slice(38, 42), slice(0, 58), rng)          # tiles 0 .. 7 (exactly 8) -> t0 = 0
    blob(crops, 7, slice(38, 42), slice(22, 80), rng)         # tiles 2 .. 9 (exactly 8) -> t0 = 2
    # rows: (0, 11) -> 0 .. 4: 2 passes; (68, 79) -> 15 .. 19: 2; every row: 5 + 5; (0, 2) -> 0 .. 2: 1; (77, 79) -> 17 .. 19: 1; (38, 41) -> 8 .. 11: 1 + 1
    assert check(monkeypatch, state, crops) == (8, 2 + 2 + 5 + 5 + 1 + 1 + 1 + 1, 0)


def test_seven_crops_both_lists(monkeypatch, state):
    rng = np.random.default_rng(12)
    crops = np.zeros((7, 80, 80, 1), np.uint8)                # crops 0 and 6 stay empty
    crops[1, :, :, 0] = rng.integers(1, 256, (80, 80))        # full of noise: no window; its rows 20 .. 39 of the batch are the aligned passes 6 .. 13
    blob(crops, 2, slice(30, 41), slice(22, 74), rng)         # exactly 8 tiles (2 .. 9); rows 6 .. 11: two windowed passes
    blob(crops, 3, slice(30, 41), slice(21, 74), rng)         # one tile wider (1 .. 9): no window; rows 66 .. 71 of the batch: passes 22, 23
    blob(crops, 4, slice(0, 9), slice(0, 11), rng)            # rows 0 .. 3: one windowed pass
    blob(crops, 5, slice(70, 80), slice(70, 80), rng)         # rows 16 .. 19: one windowed pass
    assert check(monkeypatch, state, crops) == (3, 4, 8 + 2)


def test_one_crop(monkeypatch, state):
    crops = np.zeros((1, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(35, 45), slice(25, 52), np.random.default_rng(3))
    assert check(monkeypatch, state, crops) == (1, 2, 0)      # rows (35 - 9) / 4 -> 7 .. (44 + 6) / 4 = 12: six rows


def test_tickets_of_two_slots(monkeypatch, state):
    """ellipses at every angle, as many that a ticket of either instance is two list slots (cnn_plan.h), an empty and a noise crop among them"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus * 3 + 19) // 20 + 12
    assert min(32, (20 * n + 2) // 3 // (4 * cus)) == 2, (cus, n)
    crops = weights.synthetic_crops(n, 4321).copy()
    crops[17] = 0
    crops[200, :, :, 0] = np.random.default_rng(1).integers(1, 256, (80, 80))
    (windowed, wpasses, full), skip_on, skip_nox = check(monkeypatch, state, crops, both=True)
    # (at 256 CUs: 2134 passes, three blocks of the count / list kernels, the last one partial -- the prefix across blocks is in it)
    want = listed_passes(crops)
    print("row rule: %d of %d passes listed, numpy says %d" % (skip_on[1], skip_on[0], want))
    assert skip_on[1] == want and skip_nox[1] == want
    print("%d synthetic crops: %d windowed in %d passes, %d full-width passes" % (n, windowed, wpasses, full))
    assert windowed <= n - 2 and windowed <= wpasses <= 5 * windowed and full >= 7       # the noise crop alone is 7 or 8 aligned passes
    assert windowed >= n // 2                                  # an ellipse of 18 x 5 px is at most 36 columns: 5 + 2 tiles


def test_empty_crop_out_of_range_goes_full_width(monkeypatch, state):
    """conv1's bias so large that the background itself leaves what two fp16 pieces hold: the empty crop's images are not used, no crop has a
    window, every pass is on the full-width list"""
    st = {k: v.copy() for k, v in state.items()}
    st["bn1.bias"] = np.full(16, 6000.0, np.float32)
    st["bn2.running_var"] = np.full(64, 1e8, np.float32)
    crops = weights.synthetic_crops(9, 99).copy()
    crops[4] = 0
    on, g_on, s_on = forward(monkeypatch, st, RS, crops)
    assert np.all(np.isfinite(on[0][0]))
    for name, geom in (("bit 23", NOX), ("bit 27", NOSKIP), ("bit 28", TWO)):
        other, g_other, s_other = forward(monkeypatch, st, geom, crops)
        if geom == NOX:
            assert s_other[0][:2] == ((60, 60, 0), (0, 0, 0))
        # the background itself is out of range: every crop is re-run, whichever kernel raised the flag and however it names the crops
        assert (g_on[1] or g_on[0] > 0) and (g_other[1] or g_other[0] > 0), (name, g_on, g_other)
        if geom != TWO:
            assert g_on == g_other, (name, g_on, g_other)
        assert same(on[0], other[0]), (name, float(np.abs(on[0][1] - other[0][1]).max()))
    assert s_on[0][:2] == ((60, 60, 0), (0, 0, 60))


def test_through_the_captured_graph(monkeypatch, state):
    """the same call five times (captured at the third, replayed from the fourth on), then other crops in the same buffers and a sixth call:
    bands, both lists and the counters are inside the chain, so it must follow the bytes that are in the buffer now"""
    assert os.environ.get("TREXHIP_GRAPHS", "1") != "0"
    n = 320
    crops = weights.synthetic_crops(n, 777).copy()
    crops[5] = 0
    other = np.zeros_like(crops)
    other[:, 30:50] = weights.synthetic_crops(n, 778)[:, 30:50]
    other[7, :, :, 0] = np.random.default_rng(2).integers(1, 256, (80, 80))
    on, g_on, s_on = forward(monkeypatch, state, RS, crops, calls=5, then=other)
    assert g_on == (0, False)
    for rep in range(5):
        assert s_on[rep] == s_on[0], rep
    for name, geom in (("bit 23", NOX), ("bit 27", NOSKIP), ("bit 28", TWO)):
        ref, g_ref, _ = forward(monkeypatch, state, geom, crops)
        ref2, g_ref2, _ = forward(monkeypatch, state, geom, other)
        assert g_ref == g_ref2 == (0, False), name
        for rep in range(5):
            assert same(on[rep], ref[0]), (name, rep)
        assert same(on[5], ref2[0]), name
    assert 0 < s_on[5][1][1] < s_on[0][1][1] and s_on[5][1][2] >= 7 and s_on[5][1][0] <= n - 1
