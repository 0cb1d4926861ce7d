"""The windowed listed form of conv3 (k_conv5_wpair<true, Skip3XGeom>, trex_amd/csrc/cnn_conv3p.h) computes, of every listed row pair of a crop
whose blob reaches at most 3 of a row's 5 conv3 tiles (trex_amd/csrc/cnn_skip3.h: skip3_window), only those 3 tiles, ten pairs to a pass;
k_act3_fill copies the 4 pooled columns outside the window from the empty crop's act3; the other crops take the full-width listed passes.
Every probability and logit must be, bit for bit, that of the same call with the windowed form switched off (TREXHIP_CONV_GEOM bit 21), with
the dense conv3 (bit 26) and on the two-kernel chain (bit 28), with the range guard quiet.  Bit 29 forces the role-split chain at small batches.
The counters (trexhip_identify_skip3x_stats) are held to a restatement of the rule and of the packing in numpy, from the crops' bytes."""
import os
import numpy as np
import pytest
import torch
from trex_amd import capi, weights
from cnn_skip_driver import blob, same, state  # noqa: F401  (state: the module's fixture)

pytestmark = pytest.mark.gpu

RS, NO3X, DENSE3, TWO = 1 << 29, 1 << 29 | 1 << 21, 1 << 29 | 1 << 26, 1 << 28
PAIRS, BLOCK = 10, 32


def forward(monkeypatch, st, geom, crops, classes=100, calls=1, then=None):
    """cnn_skip_driver.forward with the counters of this form: -> (probabilities, logits) of every call, guard_stats,
    (skip3_stats, skip3x_stats) of every call"""
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(geom))
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, classes))
    seg.set_identity_precision(capi.CNN_FP16X3)
    n = len(crops)
    d = torch.from_numpy(np.ascontiguousarray(crops.reshape(n, -1))).cuda()
    probs = torch.empty((n, classes), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    outs, stats = [], []
    for call in range(calls + (then is not None)):
        if call == calls:
            d.copy_(torch.from_numpy(np.ascontiguousarray(then.reshape(n, -1))).cuda())
        probs.fill_(-1.0); logits.fill_(-1.0)
        seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
        seg.synchronize()
        outs.append((probs.cpu().numpy().copy(), logits.cpu().numpy().copy()))
        stats.append((seg.skip3_stats(), seg.skip3x_stats()))
    guard = seg.guard_stats()
    seg.close()
    return outs, guard, stats


def rule(crop):
    """-> (first listed pair, listed pairs, tiles needed) of one crop, from its bytes: pair q reads the crop rows 8 q - 14 .. 8 q + 21, tile t
    the crop columns 16 t - 14 .. 16 t + 29"""
    img = crop.reshape(80, 80)
    rows, cols = np.flatnonzero(img.any(1)), np.flatnonzero(img.any(0))
    if not len(rows):
        return 0, 0, 0
    q = [k for k in range(PAIRS) if 8 * k + 21 >= rows[0] and 8 * k - 14 <= rows[-1]]
    t = [k for k in range(5) if 16 * k + 29 >= cols[0] and 16 * k - 14 <= cols[-1]]
    return q[0], len(q), len(t)


def pack(runs, slots):
    """passes of `slots` pairs and at most two runs that the run lengths of one block of crops fill, in order"""
    passes, n, nruns = 0, 0, 0
    for length in runs:
        while length:
            if n == slots or nruns == 2:
                passes, n, nruns = passes + 1, 0, 0
            take = min(length, slots - n)
            n, nruns, length = n + take, nruns + 1, length - take
    return passes + (n > 0)


def expect(crops, windows=True):
    """-> (skip3_stats' pairs, listed, passes), (crops windowed, windowed passes, full-width passes) as the listed form must report them:
    skip3_stats keeps counting by the row rule alone (every crop's pairs in passes of six), skip3x_stats says what ran"""
    rules = [rule(c) for c in crops]
    wide = wpasses = fpasses = by_rows = 0
    for b in range(0, len(crops), BLOCK):
        blk = rules[b:b + BLOCK]
        win = [windows and 0 < t <= 3 for _, _, t in blk]
        wide += sum(w and n > 0 for w, (_, n, _) in zip(win, blk))
        wpasses += pack([n for w, (_, n, _) in zip(win, blk) if w and n], 10)
        fpasses += pack([n for w, (_, n, _) in zip(win, blk) if not w and n], 6)
        by_rows += pack([n for _, n, _ in blk if n], 6)
    listed = sum(n for _, n, _ in rules)
    dense = (len(crops) * 100 + 63) // 64
    if wpasses + fpasses >= dense:
        return (PAIRS * len(crops), listed, 0), (0, 0, 0)
    return (PAIRS * len(crops), listed, by_rows), (wide, wpasses, fpasses)


def check(monkeypatch, st, crops, quiet=True):
    """-> skip3x_stats of the windowed run, held to numpy; its probabilities are those of the three other chains"""
    on, g_on, s_on = forward(monkeypatch, st, RS, crops)
    no3x, g_no3x, s_no3x = forward(monkeypatch, st, NO3X, crops)
    dense, g_dense, _ = forward(monkeypatch, st, DENSE3, crops)
    two, g_two, _ = forward(monkeypatch, st, TWO, crops)
    if quiet:
        assert g_on == g_no3x == g_dense == g_two == (0, False)
    assert np.all(np.isfinite(on[0][0])) and np.allclose(on[0][0].sum(1), 1.0, atol=1e-5)
    for name, other in (("bit 21", no3x), ("bit 26", dense), ("bit 28", two)):
        assert same(on[0], other[0]), (name, float(np.abs(on[0][1] - other[0][1]).max()), np.flatnonzero(np.any(on[0][1] != other[0][1], axis=1))[:10])
    want3, want3x = expect(crops)
    print("skip3", s_on[0][0], "skip3x", s_on[0][1], "numpy", want3, want3x)
    assert s_on[0][0][:3] == want3 and s_on[0][1] == want3x
    assert s_no3x[0][0][:3] == expect(crops, windows=False)[0] and s_no3x[0][1] == (0, 0, s_no3x[0][0][2])
    if s_no3x[0][0][2]:                                       # where both ran the listed form, skip3_stats does not see the windows at all
        assert s_on[0][0] == s_no3x[0][0]
    return s_on[0][1]


def test_one_pixel_in_row_r_column_c(monkeypatch, state):
    """a column rule that is off by one in either direction, or a wrong t0, drops a tile one of these 80 crops needs"""
    crops = np.zeros((80, 80, 80, 1), np.uint8)
    for r in range(80):
        crops[r, r, (37 * r + 11) % 80, 0] = 255
    # a pixel reaches at most 3 tiles and 5 pairs: every crop has a window, two runs to a pass
    assert check(monkeypatch, state, crops) == (80, 40, 0)


def test_bars(monkeypatch, state):
    rng = np.random.default_rng(8)
    crops = np.zeros((12, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(30, 50), slice(0, 19), rng)           # tiles 0 .. 2 exactly (column 18 <= 16 * 2 + 29, 16 * 3 - 14 = 34 > 18): t0 = 0
    blob(crops, 1, slice(30, 50), slice(30, 34), rng)          # 16 t + 29 >= 30 -> t >= 1 (t = 0 ends at 29); 16 t - 14 <= 33 -> t <= 2: tiles 1 .. 2, t0 = 1
    blob(crops, 2, slice(30, 50), slice(30, 35), rng)          # column 34 = 16 * 3 - 14: tiles 1 .. 3 exactly, t0 = 1
    blob(crops, 3, slice(30, 50), slice(46, 80), rng)          # 46 > 45 = 16 + 29: tiles 2 .. 4 exactly, t0 = 2
    blob(crops, 4, slice(30, 50), slice(45, 80), rng)          # column 45: tiles 1 .. 4, four tiles: no window
    blob(crops, 5, slice(30, 50), slice(10, 70), rng)          # five tiles
    blob(crops, 6, slice(0, 80), slice(40, 42), rng)           # ten pairs, tiles 1 .. 3: one run fills a windowed pass
    blob(crops, 7, slice(0, 80), slice(0, 2), rng)             # ten pairs, tile 0 alone
    blob(crops, 8, slice(10, 50), slice(78, 80), rng)          # pairs 0 .. 7 (8 q - 14 <= 49), tile 4 alone -> t0 = 2
    blob(crops, 9, slice(30, 80), slice(50, 60), rng)          # pairs 2 .. 9: the run splits by rows between two passes
    blob(crops, 10, slice(0, 80), slice(0, 80), rng)           # every pair, every tile
    blob(crops, 11, slice(78, 80), slice(0, 1), rng)           # the last rows, the first column
    got = check(monkeypatch, state, crops)
    assert got[0] == 9


def test_mixed_batch_partial_block(monkeypatch, state):
    """empty, noise, narrow and wide crops: both lists are filled, and the last block of 32 crops is partial"""
    n = 327
    rng = np.random.default_rng(21)
    crops = weights.synthetic_crops(n, 2024).copy()
    for i in range(0, n, 7):
        crops[i] = 0
    for i in range(3, n, 41):
        crops[i, :, :, 0] = rng.integers(1, 256, (80, 80))
    for i in range(5, n, 3):                                    # narrow and tall
        crops[i] = 0
        x0 = int(rng.integers(0, 70))
        blob(crops, i, slice(int(rng.integers(0, 30)), int(rng.integers(50, 80))), slice(x0, x0 + int(rng.integers(1, 10))), rng)
    wide, wpasses, full = check(monkeypatch, state, crops)
    assert wide > 80 and wpasses > 0 and full > 0


def test_stale_buffers_and_the_replayed_graph(monkeypatch, state):
    """a noise batch first, then -- in the same buffers, through the graph that was captured on other crops -- narrow crops: act3 columns outside
    the windows that the fill did not write would hold the noise batch's values"""
    assert os.environ.get("TREXHIP_GRAPHS", "1") != "0"
    n = 320
    rng = np.random.default_rng(4)
    noise = rng.integers(1, 256, (n, 80, 80, 1)).astype(np.uint8)
    narrow = np.zeros_like(noise)
    for i in range(n):
        x0 = int(rng.integers(0, 72))
        blob(narrow, i, slice(int(rng.integers(0, 40)), int(rng.integers(40, 80))), slice(x0, x0 + 8), rng)
    narrow[9] = 0
    narrow[100] = noise[100]
    on, g_on, s_on = forward(monkeypatch, state, RS, noise, calls=5, then=narrow)
    assert g_on == (0, False)
    assert s_on[0][1] == (0, 0, 0) and s_on[0][0][2] == 0      # noise: the dense kernel runs
    want3, want3x = expect(narrow)
    assert s_on[5][0][:3] == want3 and s_on[5][1] == want3x and want3x[1] > 0
    for name, geom in (("bit 21", NO3X), ("bit 26", DENSE3), ("bit 28", TWO)):
        ref, g_ref, _ = forward(monkeypatch, state, geom, noise)
        ref2, g_ref2, _ = forward(monkeypatch, state, geom, narrow)
        assert g_ref == g_ref2 == (0, False), name
        for rep in range(5):
            assert same(on[rep], ref[0]), (name, rep)
        assert same(on[5], ref2[0]), name


@pytest.mark.parametrize("n", [1024, 1056])
def test_around_the_small_batch_threshold(monkeypatch, state, n):
    """1024 crops: the dense fc1 and the small head read whole act3 -- the fill copies pairs and columns; above: the listed fc1 and k_head"""
    crops = weights.synthetic_crops(n, 515).copy()
    rng = np.random.default_rng(n)
    for i in range(0, n, 2):
        crops[i] = 0
        x0 = int(rng.integers(0, 75))
        blob(crops, i, slice(int(rng.integers(0, 60)), int(rng.integers(60, 80))), slice(x0, x0 + 5), rng)
    wide, wpasses, full = check(monkeypatch, state, crops)
    assert wide >= n // 2 and wpasses > 0


def test_empty_crop_out_of_range_has_no_windows(monkeypatch, state):
    """conv1's bias so large that the background itself leaves what two fp16 pieces hold: the empty crop's images are not used, every pair is
    listed and no crop has a window"""
    st = {k: v.copy() for k, v in state.items()}
    st["bn1.bias"] = np.full(16, 6000.0, np.float32)
    st["bn2.running_var"] = np.full(64, 1e8, np.float32)
    crops = np.zeros((9, 80, 80, 1), np.uint8)
    rng = np.random.default_rng(6)
    for i in range(8):
        blob(crops, i, slice(30, 40), slice(8 * i, 8 * i + 6), rng)
    on, g_on, s_on = forward(monkeypatch, st, RS, crops)
    assert np.all(np.isfinite(on[0][0]))
    assert s_on[0][1][:2] == (0, 0)
    for name, geom in (("bit 21", NO3X), ("bit 26", DENSE3), ("bit 28", TWO)):
        other, g_other, s_other = forward(monkeypatch, st, geom, crops)
        assert (g_on[1] or g_on[0] > 0) and (g_other[1] or g_other[0] > 0), (name, g_on, g_other)
        assert same(on[0], other[0]), (name, float(np.abs(on[0][1] - other[0][1]).max()))
