"""The role-split conv1+conv2 kernel computes only the passes whose crop rows hold a non-zero byte and copies the rows of the others from the
image of an all-zero crop (trex_amd/csrc/cnn_skip.h): every result must be, bit for bit, that of a run which computes every pass
(TREXHIP_CONV_GEOM bit 27) and that of the two-kernel chain (bit 28).  Bit 29 forces the role-split kernel at small batches."""
import os
import numpy as np
import pytest
import torch
from trex_amd import weights
from cnn_skip_driver import blob, forward, same, state  # noqa: F401  (state: the module's fixture)

pytestmark = pytest.mark.gpu

RS, NOSKIP, TWO = 1 << 29, 1 << 29 | 1 << 27, 1 << 28
V3_ROWB = 10240


def check(monkeypatch, st, crops):
    on, g_on, stats = forward(monkeypatch, st, RS, crops)
    off, g_off, _ = forward(monkeypatch, st, NOSKIP, crops)
    two, g_two, _ = forward(monkeypatch, st, TWO, crops)
    s_on = stats[-1].skip
    assert g_on == g_off == g_two == (0, False)              # background activations in range: nothing is re-run
    assert np.all(np.isfinite(on[0][0])) and np.allclose(on[0][0].sum(1), 1.0, atol=1e-5)
    assert same(on[0], off[0]), float(np.abs(on[0][1] - off[0][1]).max())
    assert same(on[0], two[0]), float(np.abs(on[0][1] - two[0][1]).max())
    passes, listed, filled = s_on
    assert passes == (20 * len(crops) + 2) // 3 and 0 <= listed <= passes
    return s_on


def test_one_empty_crop_is_all_fill(monkeypatch, state):
    passes, listed, filled = check(monkeypatch, state, np.zeros((1, 80, 80, 1), np.uint8))
    assert (passes, listed, filled) == (7, 0, 20 * V3_ROWB)


def test_one_pixel_in_row_r_of_crop_r(monkeypatch, state):
    """a band that is off by one row in either direction drops a pass that one of these 80 crops needs"""
    crops = np.zeros((80, 80, 80, 1), np.uint8)
    for r in range(80):
        crops[r, r, (37 * r + 11) % 80, 0] = 255
    passes, listed, filled = check(monkeypatch, state, crops)
    assert 80 <= listed <= 3 * 80                             # 2 to 4 rows per crop: one to three passes each
    assert filled >= (20 * 80 - 3 * listed) * V3_ROWB


def test_seven_crops_passes_straddle(monkeypatch, state):
    rng = np.random.default_rng(12)
    crops = np.zeros((7, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(0, 9), slice(20, 60), rng)           # touches row 0
    blob(crops, 1, slice(70, 80), slice(5, 75), rng)          # touches row 79: its last pass holds row 0 of crop 2
    blob(crops, 2, slice(0, 3), slice(0, 80), rng)
    crops[3, :, :, 0] = rng.integers(0, 256, (80, 80))        # full of noise
    blob(crops, 5, slice(33, 47), slice(30, 50), rng)         # crop 4 stays empty
    blob(crops, 6, slice(76, 80), slice(0, 10), rng)          # the last, partial pass
    passes, listed, filled = check(monkeypatch, state, crops)
    assert passes == 47 and 7 <= listed < passes and filled > 0


def test_320_crops_tickets_cross_gaps(monkeypatch, state):
    """ellipses at every angle, as many that a ticket is two list slots (cnn_plan.h: pk2 = passes / (4 workgroups), one workgroup per CU; 320
    crops = 2134 passes on 256 CUs), with gaps of skipped passes inside and between tickets"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus * 3 + 19) // 20 + 12
    n_pass = (20 * n + 2) // 3
    assert min(32, n_pass // (4 * cus)) == 2, (cus, n, n_pass)
    crops = weights.synthetic_crops(n, 4321).copy()
    crops[17] = 0
    crops[200, :, :, 0] = np.random.default_rng(1).integers(0, 256, (80, 80))
    passes, listed, filled = check(monkeypatch, state, crops)
    assert passes == n_pass and passes // 4 < listed < passes
    print("%d synthetic crops: %d of %d passes listed, %d bytes filled" % (n, listed, passes, filled))


def test_empty_crop_out_of_range_lists_every_pass(monkeypatch, state):
    """conv1's bias so large that the background itself leaves what two fp16 pieces hold: the empty crop's image is not used, every pass is
    computed, and the range guard does what it does with skipping switched off"""
    st = {k: v.copy() for k, v in state.items()}
    st["bn1.bias"] = np.full(16, 6000.0, np.float32)
    st["bn2.running_var"] = np.full(64, 1e8, np.float32)      # bring the scale back down behind conv2
    crops = weights.synthetic_crops(9, 99).copy()
    crops[4] = 0
    on, g_on, stats = forward(monkeypatch, st, RS, crops)
    off, g_off, _ = forward(monkeypatch, st, NOSKIP, crops)
    s_on = stats[-1].skip
    assert g_on == g_off and (g_on[1] or g_on[0] > 0), (g_on, g_off)
    assert np.all(np.isfinite(on[0][0]))
    assert same(on[0], off[0])
    assert s_on == (60, 60, 0)


def test_through_the_captured_graph(monkeypatch, state):
    """the same call five times -- cnn.hip captures a call's chain when its (buffers, n, precision) key comes the third time and replays it from
    the fourth on, unless TREXHIP_GRAPHS=0 --, then other crops in the same buffers and a sixth call: bands, list and fill are inside the
    chain, so it must follow the bytes that are in the buffer now.  (The library has no counter of replays; that small chains are replayed is
    what tests/test_cnn_gpu.py::test_replayed_chain_follows_new_inputs_and_precision_changes rests on as well.)"""
    assert os.environ.get("TREXHIP_GRAPHS", "1") != "0"
    n = 320                                                   # <= 6400: above that the chain is never captured
    crops = weights.synthetic_crops(n, 777).copy()
    crops[5] = 0
    other = np.zeros_like(crops)
    other[:, 30:50] = weights.synthetic_crops(n, 778)[:, 30:50]      # every blob cut down to rows 30 .. 49: fewer passes than before
    on, g_on, stats = forward(monkeypatch, state, RS, crops, calls=5, then=other)
    s_on = [s.skip for s in stats]
    off, g_off, _ = forward(monkeypatch, state, NOSKIP, crops)
    off2, g_off2, _ = forward(monkeypatch, state, NOSKIP, other)
    assert g_on == g_off == g_off2 == (0, False)
    for rep in range(5):
        assert same(on[rep], off[0]), rep
        assert s_on[rep] == s_on[0], rep
    assert same(on[5], off2[0])
    assert 0 < s_on[5][1] < s_on[0][1] < s_on[0][0]
