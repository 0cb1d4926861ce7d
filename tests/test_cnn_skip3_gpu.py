"""conv3 (k_conv5_wpair) computes only the row pairs that read a V3 row with a blob in it, six listed pairs to a pass, and copies the other row
pairs from the act3 of an all-zero crop (trex_amd/csrc/cnn_skip3.h): every result must be, bit for bit, that of a run whose conv3 is the dense
kernel (TREXHIP_CONV_GEOM bit 26) and that of the two-kernel chain (bit 28).  Bit 29 forces the role-split chain at small batches."""
import os
import numpy as np
import pytest
import torch
from trex_amd import weights
from cnn_skip_driver import blob, forward, same, state  # noqa: F401  (state: the module's fixture)

pytestmark = pytest.mark.gpu

RS, DENSE3, TWO = 1 << 29, 1 << 29 | 1 << 26, 1 << 28
PAIRB = 10 * 128 * 4          # bytes of one row pair of act3


def pairs_of(crop):
    """the row pairs of a crop that read one of its non-zero rows: pair q reads the crop rows 8 q - 14 .. 8 q + 21"""
    rows = np.flatnonzero(crop.reshape(80, -1).any(1))
    return [q for q in range(10) if len(rows) and rows[0] <= 8 * q + 21 and rows[-1] >= 8 * q - 14]


def check(monkeypatch, st, crops):
    on, g_on, stats = forward(monkeypatch, st, RS, crops)
    off, g_off, stats_off = forward(monkeypatch, st, DENSE3, crops)
    two, g_two, _ = forward(monkeypatch, st, TWO, crops)
    s_on, s_off = stats[-1].skip3, stats_off[-1].skip3
    assert g_on == g_off == g_two == (0, False)              # background activations in range: nothing is re-run
    assert np.all(np.isfinite(on[0][0])) and np.allclose(on[0][0].sum(1), 1.0, atol=1e-5)
    assert same(on[0], off[0]), float(np.abs(on[0][1] - off[0][1]).max())
    assert same(on[0], two[0]), float(np.abs(on[0][1] - two[0][1]).max())
    pairs, listed, passes, filled = s_on
    want = sum(len(pairs_of(c)) for c in crops)
    print("%d crops: %d of %d pairs listed in %d passes, %d bytes filled" % (len(crops), listed, pairs, passes, filled))
    assert pairs == 10 * len(crops) and listed == want
    assert s_off == (0, 0, 0, 0)                             # bit 26: nothing is listed, nothing is filled
    if passes:                                               # the listed form ran
        assert (listed + 5) // 6 <= passes <= listed and filled == (pairs - listed) * PAIRB
    else:
        assert filled == (0 if listed else pairs * PAIRB)
    return s_on


def test_one_empty_crop_is_all_fill(monkeypatch, state):
    assert check(monkeypatch, state, np.zeros((1, 80, 80, 1), np.uint8)) == (10, 0, 0, 10 * PAIRB)


def test_one_pixel_in_row_r_of_crop_r(monkeypatch, state):
    """a range that is off by one pair in either direction at any row drops a pair that one of these 80 crops needs (or its bits differ);
    runs of 2 to 5 pairs, clipped at both crop edges"""
    crops = np.zeros((80, 80, 80, 1), np.uint8)
    for r in range(80):
        crops[r, r, (37 * r + 11) % 80, 0] = 255
    assert {len(pairs_of(c)) for c in crops} == {2, 3, 4, 5}
    pairs, listed, passes, filled = check(monkeypatch, state, crops)
    assert passes > 0


def test_seven_crops_passes_straddle(monkeypatch, state):
    rng = np.random.default_rng(12)
    crops = np.zeros((7, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(0, 9), slice(20, 60), rng)           # touches row 0
    blob(crops, 1, slice(70, 80), slice(5, 75), rng)          # touches row 79
    blob(crops, 2, slice(0, 3), slice(0, 80), rng)
    crops[3, :, :, 0] = rng.integers(0, 256, (80, 80))        # full of noise
    blob(crops, 5, slice(33, 47), slice(30, 50), rng)         # crop 4 stays empty
    blob(crops, 6, slice(76, 80), slice(0, 10), rng)          # the last, partial pass
    pairs, listed, passes, filled = check(monkeypatch, state, crops)
    assert [len(pairs_of(c)) for c in crops] == [3, 3, 3, 10, 0, 6, 3]
    assert passes == 5                                        # 3 + 3 | 3 + 3 | 6 | 1 + 5 | 1 + 3


def test_a_third_run_ends_the_pass(monkeypatch, state):
    rng = np.random.default_rng(4)
    crops = np.zeros((3, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(25, 46), slice(10, 70), rng)         # pairs 1 .. 7
    crops[1, 40, 17, 0] = 200                                 # pairs 3 .. 6
    crops[2, :, :, 0] = rng.integers(0, 256, (80, 80))
    assert [pairs_of(c) for c in crops] == [list(range(1, 8)), [3, 4, 5, 6], list(range(10))]
    # 6 | 1 + 4: the pass that holds A's last pair and B's four ends there | 6 | 4
    assert check(monkeypatch, state, crops) == (30, 21, 4, 9 * PAIRB)


def test_320_crops(monkeypatch, state):
    crops = weights.synthetic_crops(320, 4321).copy()
    crops[17] = 0
    crops[200, :, :, 0] = np.random.default_rng(1).integers(0, 256, (80, 80))
    pairs, listed, passes, filled = check(monkeypatch, state, crops)
    assert passes > 0 and pairs // 4 < listed < pairs


def test_tickets_of_four_list_slots(monkeypatch, state):
    """as many crops that the listed passes go out in tickets of four consecutive list slots (16 per workgroup and more), with gaps inside and
    between the tickets"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    base = weights.synthetic_crops(320, 99).copy()
    base[5] = 0
    n = 20 * cus
    crops = np.concatenate([np.roll(base, 3 * k, axis=1) for k in range((n + 319) // 320)])[:n]
    pairs, listed, passes, filled = check(monkeypatch, state, crops)
    assert passes >= 16 * cus, (passes, cus)


def test_empty_crop_out_of_range_lists_every_pair(monkeypatch, state):
    """conv1's bias so large that the background itself leaves what two fp16 pieces hold: the empty crop's images are not used, every pair is
    listed -- which is more passes than the dense kernel's, so that one runs -- and the range guard does what it does without the list"""
    st = {k: v.copy() for k, v in state.items()}
    st["bn1.bias"] = np.full(16, 6000.0, np.float32)
    st["bn2.running_var"] = np.full(64, 1e8, np.float32)      # bring the scale back down behind conv2
    crops = weights.synthetic_crops(9, 99).copy()
    crops[4] = 0
    on, g_on, stats = forward(monkeypatch, st, RS, crops)
    off, g_off, _ = forward(monkeypatch, st, DENSE3, crops)
    s_on = stats[-1].skip3
    assert g_on == g_off and (g_on[1] or g_on[0] > 0), (g_on, g_off)
    assert np.all(np.isfinite(on[0][0]))
    assert same(on[0], off[0])
    assert s_on == (90, 90, 0, 0)


def test_through_the_captured_graph(monkeypatch, state):
    """the same call five times -- the chain is captured when its key comes the third time and replayed from the fourth on --, then other crops in
    the same buffers and a sixth call: the list, the fill and the choice of the kernel are inside the chain and follow the bytes in the buffer"""
    assert os.environ.get("TREXHIP_GRAPHS", "1") != "0"
    n = 320
    crops = weights.synthetic_crops(n, 777).copy()
    crops[5] = 0
    other = np.zeros_like(crops)
    other[:, 30:50] = weights.synthetic_crops(n, 778)[:, 30:50]      # every blob cut down to rows 30 .. 49: fewer pairs than before
    on, g_on, stats = forward(monkeypatch, state, RS, crops, calls=5, then=other)
    s_on = [s.skip3 for s in stats]
    off, g_off, _ = forward(monkeypatch, state, DENSE3, crops)
    off2, g_off2, _ = forward(monkeypatch, state, DENSE3, other)
    assert g_on == g_off == g_off2 == (0, False)
    for rep in range(5):
        assert same(on[rep], off[0]), rep
        assert s_on[rep] == s_on[0], rep
    assert same(on[5], off2[0])
    assert 0 < s_on[5][1] < s_on[0][1] < s_on[0][0] and 0 < s_on[5][2] < s_on[0][2]


def test_noise_takes_the_dense_kernel(monkeypatch, state):
    """every pair of every crop is listed: six-pair passes would be 6.7 % more than the dense kernel's, the device chooses the dense one"""
    crops = np.random.default_rng(8).integers(0, 256, (64, 80, 80, 1)).astype(np.uint8)
    assert check(monkeypatch, state, crops) == (640, 640, 0, 0)
