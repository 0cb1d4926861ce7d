"""The listed forms of conv3 on passes of TILE slots (k_conv5_wpair<true, Skip3TGeom> and <true, Skip3TXGeom>, trex_amd/csrc/cnn_conv3p.h): a pass
is up to 64 consecutive tiles of its list's pair sequence (trex_amd/csrc/cnn_skip3.h), begun and ended at any even tile of a pair.  Every probability and
logit must be, bit for bit, that of the same call on passes of whole pairs (TREXHIP_CONV_GEOM bit 20), with the dense conv3 (bit 26) and
without windows (bit 21, where every listed pair goes into passes of tile slots), with the range guard quiet.  Bit 29 forces the role-split
chain at small batches.  The passes that ran (trexhip_identify_skip3_ran) are held to a restatement of the rule and of the packing in numpy,
from the crops' bytes, and so are the counters that keep counting passes of whole pairs; each case asserts from the restatement that the
passes it is there for occurred.  (A windowed pass of tiles may touch 12 pairs, 32 rows: no pass closes at 62 tiles, cnn_skip3.h.)"""
import os
import numpy as np
import pytest
import torch
from trex_amd import capi, weights
from cnn_skip_driver import blob, same, state  # noqa: F401  (state: the module's fixture)

pytestmark = pytest.mark.gpu

RS = 1 << 29
PAIR_SLOTS, NO3X, DENSE3 = RS | 1 << 20, RS | 1 << 21, RS | 1 << 26
PAIRS, BLOCK, TPP, MAXP = 10, 32, 10, 8


def forward(monkeypatch, st, geom, crops, classes=100, calls=1, then=None):
    """-> (probabilities, logits) of every call, guard_stats, (skip3_stats, skip3x_stats, skip3_ran) of every call"""
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
        stats.append((seg.skip3_stats(), seg.skip3x_stats(), seg.skip3_ran()))
    guard = seg.guard_stats()
    seg.close()
    return outs, guard, stats


def rule(crop):
    """-> (listed pairs, tiles needed) of one crop, from its bytes: pair q reads the crop rows 8 q - 14 .. 8 q + 21, tile t the crop columns
    16 t - 14 .. 16 t + 29"""
    img = crop.reshape(80, 80)
    rows, cols = np.flatnonzero(img.any(1)), np.flatnonzero(img.any(0))
    if not len(rows):
        return 0, 0
    return (sum(8 * k + 21 >= rows[0] and 8 * k - 14 <= rows[-1] for k in range(PAIRS)),
            sum(16 * k + 29 >= cols[0] and 16 * k - 14 <= cols[-1] for k in range(5)))


def pack_pairs(runs, slots):
    """passes of `slots` whole pairs and at most two runs that the run lengths of one block of crops fill, in order"""
    passes, n, nruns = 0, 0, 0
    for length in runs:
        while length:
            if n == slots or nruns == 2:
                passes, n, nruns = passes + 1, 0, 0
            take = min(length, slots - n)
            n, nruns, length = n + take, nruns + 1, length - take
    return passes + (n > 0)


def pack_tiles(runs, TPP=TPP, MAXP=MAXP):
    """the passes of up to 64 consecutive tiles, at most two runs and at most MAXP pairs touched that the run lengths (pairs of TPP tiles) of one
    block of crops fill, tile pair by tile pair: -> [(tiles into its first pair the pass begins, its tiles, its runs)]"""
    out, n, nruns, pairs, last, start = [], 0, 0, 0, None, 0
    for r, length in enumerate(runs):
        for q in range(length):
            for place in range(0, TPP, 2):
                new_run, new_pair = last is None or last[0] != r, last is None or last != (r, q)
                if n and (n == 64 or (new_run and nruns == 2) or (new_pair and pairs == MAXP)):
                    out.append((start, n, nruns))
                    n, nruns, pairs, last, new_run, new_pair = 0, 0, 0, None, True, True
                if n == 0:
                    start = place
                nruns, pairs, n, last = nruns + new_run, pairs + new_pair, n + 2, (r, q)
    if n:
        out.append((start, n, nruns))
    return out


def expect(crops, windows=True, tiled=True):
    """-> skip3_stats[:3], skip3x_stats, skip3_ran as the call must report them, and the full-width passes of tile slots in order (expect.windowed:
    the windowed ones of the last call)"""
    rules = [rule(c) for c in crops]
    wide = wpasses = fpasses = by_rows = 0
    tiles, wtiles = [], []
    for b in range(0, len(crops), BLOCK):
        blk = rules[b:b + BLOCK]
        win = [windows and 0 < t <= 3 for _, t in blk]
        wide += sum(w and n > 0 for w, (n, _) in zip(win, blk))
        wpasses += pack_pairs([n for w, (n, _) in zip(win, blk) if w and n], 10)
        wtiles += pack_tiles([n for w, (n, _) in zip(win, blk) if w and n], 6, 12)
        full = [n for w, (n, _) in zip(win, blk) if not w and n]
        fpasses += pack_pairs(full, 6)
        tiles += pack_tiles(full)
        by_rows += pack_pairs([n for n, _ in blk if n], 6)
    listed = sum(n for n, _ in rules)
    expect.windowed = wtiles
    if wpasses + fpasses >= (len(crops) * 100 + 63) // 64:      # the choice stays one between passes of whole pairs and the dense kernel's
        return (PAIRS * len(crops), listed, 0), (0, 0, 0), (0, 0), []
    return (PAIRS * len(crops), listed, by_rows), (wide, wpasses, fpasses), (len(wtiles), len(tiles)) if tiled else (wpasses, fpasses), tiles


def check(monkeypatch, st, crops):
    """-> the full-width passes of tile slots the call must have walked; its counters are held to numpy, its results to the three other forms"""
    on, g_on, s_on = forward(monkeypatch, st, RS, crops)
    want3, want3x, ran, tiles = expect(crops)
    print("skip3", s_on[0][0], "skip3x", s_on[0][1], "ran", s_on[0][2], "numpy", want3, want3x, ran)
    assert g_on == (0, False)
    assert np.all(np.isfinite(on[0][0])) and np.allclose(on[0][0].sum(1), 1.0, atol=1e-5)
    assert s_on[0][0][:3] == want3 and s_on[0][1] == want3x and s_on[0][2] == ran
    for name, geom in (("bit 20", PAIR_SLOTS), ("bit 26", DENSE3), ("bit 21", NO3X)):
        other, g_other, s_other = forward(monkeypatch, st, geom, crops)
        assert g_other == (0, False), name
        assert same(on[0], other[0]), (name, float(np.abs(on[0][1] - other[0][1]).max()), np.flatnonzero(np.any(on[0][1] != other[0][1], axis=1))[:10])
        if geom == PAIR_SLOTS:                                # what ran is what the old counters count
            assert s_other[0][0][:3] == want3 and s_other[0][1] == want3x and s_other[0][2] == want3x[1:]
        if geom == NO3X:
            w3, w3x, wran, _ = expect(crops, windows=False)
            assert s_other[0][0][:3] == w3 and s_other[0][2] == wran and s_other[0][1] == (0, 0, w3[2])
    return tiles


def wide_crops(lengths, rng, n=None):
    """crops whose blob spans every column and lengths[i] row pairs (0: an empty crop), from pair 10 - lengths[i] on (a blob at the crop's last row is read by two pairs: no length 1)"""
    crops = np.zeros((n or len(lengths), 80, 80, 1), np.uint8)
    for i, k in enumerate(lengths):
        if k:
            # the pairs q >= 10 - k: rows from 8 (10 - k) + 22 - 8 on are read by pair 10 - k and not by the one above it
            blob(crops, i, slice(0 if k == PAIRS else 8 * (PAIRS - k) + 14, 80), slice(0, 80), rng)
    return crops


def test_every_offset_cut_pairs_and_a_third_run(monkeypatch, state):
    """runs of 10, 7, 3 and 2 pairs between empty crops: passes that begin 0, 2, 4, 6 and 8 tiles into a pair, pairs cut between two passes
    (every pass is a ticket of its own at this size: each cut is one between two workgroups), and passes closed by a third run"""
    rng = np.random.default_rng(3)
    lengths = [10, 10, 0, 10, 10, 0, 10, 0, 0, 7, 7, 0, 7, 3, 0, 2, 2, 2, 0, 7, 10, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    crops = wide_crops(lengths, rng)
    assert [rule(c) for c in crops] == [(k, 5 if k else 0) for k in lengths]
    tiles = check(monkeypatch, state, crops)
    assert {o for o, _, _ in tiles} == {0, 2, 4, 6, 8}
    assert any((o + n) % TPP for o, n, _ in tiles[:-1])                                      # a pair cut between two passes
    assert any(n < 64 and runs == 2 for o, n, runs in tiles[:-1])                            # closed by a third run


def test_windowed_passes_at_every_offset(monkeypatch, state):
    """narrow crops (a window of 3 tiles) of 10, 8 and 3 pairs: windowed passes that begin 0, 2 and 4 tiles into a pair, one of them with all 12
    pairs = 32 rows, pairs cut between passes, a pass closed by a third run"""
    rng = np.random.default_rng(9)
    lengths = [10, 10, 10, 10, 0, 8, 8, 8, 8, 8, 0, 3, 3, 3, 10, 0, 0, 0, 0, 0]
    crops = wide_crops(lengths, rng)
    crops[:, :, :36] = 0
    crops[:, :, 44:] = 0
    assert [rule(c) for c in crops] == [(k, 3 if k else 0) for k in lengths]
    assert check(monkeypatch, state, crops) == []
    expect(crops)
    wt = expect.windowed
    assert {o for o, _, _ in wt} == {0, 2, 4} and any(o == 4 and n == 64 for o, n, _ in wt)
    assert any((o + n) % 6 for o, n, _ in wt[:-1]) and any(n < 64 and runs == 2 for o, n, runs in wt[:-1])


def test_a_last_pass_of_two_tiles(monkeypatch, state):
    """13 listed pairs: 64 + 64 + 2 tiles"""
    rng = np.random.default_rng(4)
    crops = wide_crops([10, 3] + [0] * 6, rng)
    tiles = check(monkeypatch, state, crops)
    assert tiles == [(0, 64, 1), (4, 64, 2), (8, 2, 1)]


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33])
def test_batches_around_the_block_of_32_crops(monkeypatch, state, n):
    """a pass never holds pairs of two blocks of 32 crops: crop 31's last tiles close a pass, crop 32 begins one"""
    rng = np.random.default_rng(n)
    crops = wide_crops([6 if i % 2 == 0 or i >= 30 else 0 for i in range(n)], rng)
    tiles = check(monkeypatch, state, crops)
    assert len(tiles) > 0 and sum(t for _, t, _ in tiles) == 60 * sum(1 for i in range(n) if i % 2 == 0 or i >= 30)
    if n == 33:
        assert tiles[-1] == (0, 60, 1)


def test_tickets_of_four_passes(monkeypatch, state):
    """5120 crops, most of them wide: more than 16 passes per workgroup, so the first 7/8 of the passes go out in tickets of four -- pairs are cut
    inside a ticket and at the boundary between two"""
    n = 5120
    rng = np.random.default_rng(11)
    lengths = [int(k) for k in rng.integers(5, 9, n)]
    crops = wide_crops(lengths, rng)
    for i in range(0, n, 5):                                   # narrow ones: the windowed instance has a list as well
        crops[i] = 0
        blob(crops, i, slice(20, 60), slice(36, 44), rng)
    tiles = check(monkeypatch, state, crops)
    assert len(tiles) >= 16 * 256
    big = (len(tiles) * 7 // 8) // 4 * 4
    assert any(o for i, (o, _, _) in enumerate(tiles[:big]) if i % 4 == 0) and any(o for i, (o, _, _) in enumerate(tiles[:big]) if i % 4)


def test_stale_lists_and_the_replayed_graph(monkeypatch, state):
    """below the small-batch threshold the chain is captured and replayed; then, in the same buffers and through the same graph, other crops:
    descriptors, row words and act3 of the first batch must not show"""
    assert os.environ.get("TREXHIP_GRAPHS", "1") != "0"
    n = 320
    rng = np.random.default_rng(6)
    first = wide_crops([int(k) for k in rng.integers(4, 10, n)], rng)
    second = wide_crops([int(k) for k in rng.integers(0, 8, n)], rng)
    for i in range(0, n, 3):
        second[i] = 0
        blob(second, i, slice(int(rng.integers(0, 40)), int(rng.integers(40, 80))), slice(30, 38), rng)
    on, g_on, s_on = forward(monkeypatch, state, RS, first, calls=5, then=second)
    assert g_on == (0, False)
    for crops, calls in ((first, range(5)), (second, [5])):
        want3, want3x, ran, tiles = expect(crops)
        assert ran[1] > 0 and any(o for o, _, _ in tiles)
        for c in calls:
            assert s_on[c][0][:3] == want3 and s_on[c][1] == want3x and s_on[c][2] == ran, c
        for name, geom in (("bit 20", PAIR_SLOTS), ("bit 26", DENSE3), ("bit 21", NO3X)):
            ref, g_ref, _ = forward(monkeypatch, state, geom, crops)
            assert g_ref == (0, False), name
            for c in calls:
                assert same(on[c], ref[0]), (name, c)
