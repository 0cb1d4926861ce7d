"""The inputs of tests/test_cnn_reach_gpu.py (tests/cnn_reach_cases.py), on the CPU: the builder is deterministic, every crop of a batch is the
pool crop its index names, the structural crops lie where the builder's docstring says -- re-derived here from 393216, 10240, 20, 32 and 8192 --,
the pool stays inside the fp16 range guard's limits by the fp32 oracle's stage maxima, and the form of conv3 each batch gets follows from the
inputs: counted with the rules restated in cnn_reach_cases, not observed from the device."""
import numpy as np
import pytest
import torch

from oracle import cnn_oracle
from trex_amd import weights
import cnn_reach_cases as rc

N_STEP, N_FITS, N_OUT = 25600, 32766, 32767
REACH_ROWS, ROWB, V3_ROWS, BLOCK, GROUP = 393216, 10240, 20, 32, 8192


def test_pool_is_what_the_docstring_says():
    pool, kinds = rc.pool(), rc.kinds()
    assert pool.shape == (509, 80, 80, 1) and pool.dtype == np.uint8
    assert {k: int((kinds == k).sum()) for k in np.unique(kinds)} == {"synth": 460, "band": 19, "pixel": 10, "zero": 4, "noise": 16}
    # distinct but for the four empty ones
    assert len({c.tobytes() for c in pool}) == 509 - 3
    assert not pool[rc.ids("zero")].any()
    heights = [int(c.reshape(80, -1).any(1).sum()) for c in pool[rc.ids("synth")]]
    assert 9 <= min(heights) and max(heights) <= 59, (min(heights), max(heights))
    assert all(1 <= rc.band_of(c)[1] - rc.band_of(c)[0] + 1 <= 20 for c in pool[rc.ids("band")])
    assert sorted(rc.band_of(c)[0] for c in pool[rc.ids("pixel")]) == [0, 9, 10, 21, 22, 40, 58, 69, 70, 79]
    assert all(int((c != 0).sum()) == 1 for c in pool[rc.ids("pixel")])
    assert all(len(rc.pairs_of(c)) == 10 for c in pool[rc.ids("noise")])
    # the one-pixel rows are where the rules change their answer: every length and position of a run at both crop edges
    assert {tuple(rc.pairs_of(pool[rc.pixel_id(r)])) for r in rc.PIXEL_ROWS} == {(0, 1), (0, 1, 2), (0, 1, 2, 3), (0, 1, 2, 3, 4), (1, 2, 3, 4), (3, 4, 5, 6),
                                                                                   (5, 6, 7, 8, 9), (6, 7, 8, 9), (7, 8, 9), (8, 9)}


def test_builder_is_deterministic_and_idx_names_equal_bytes():
    rc._pool.cache_clear(); rc.indices.cache_clear()
    first = rc.pool().copy()
    i1 = {k: rc.indices(k, N_STEP).copy() for k in ("S", "S2", "N", "M")}
    rc._pool.cache_clear(); rc.indices.cache_clear()
    assert rc.pool().tobytes() == first.tobytes()
    for k in i1:
        crops, idx = rc.batch(k, N_STEP)
        assert np.array_equal(idx, i1[k]) and crops.shape == (N_STEP, 80, 80, 1)
        assert 0 <= idx.min() and idx.max() < 509
        for i in range(0, N_STEP, 997):
            assert crops[i].tobytes() == first[idx[i]].tobytes()
        assert crops.tobytes() == first[idx].tobytes()
    assert not np.isin(rc.kinds()[i1["S"]], "noise").any() and not np.isin(rc.kinds()[i1["S2"]], "noise").any()
    assert (rc.kinds()[i1["N"]] == "noise").all()
    # every crop that is not noise occurs in S, at every residue of a block
    assert set(i1["S"]) == set(rc.ids("synth", "band", "pixel", "zero"))
    # a smaller batch is the larger one's head but for the overrides at its own end
    small = rc.indices("S", 3200)
    assert np.array_equal(small[1:3197], i1["S"][1:3197])


def test_walk_restates_the_packing():
    """the pass counts test_cnn_skip3_gpu.py holds the device to (test_seven_crops_passes_straddle, test_a_third_run_ends_the_pass)"""
    assert len(rc.listed_passes([(0, 3), (7, 3), (0, 3), (0, 10), (0, 0), (2, 6), (7, 3)])) == 5
    assert len(rc.listed_passes([(1, 7), (3, 4), (0, 10)])) == 4
    assert len(rc.listed_passes([(0, 10)] * 64)) == 2 * ((320 + 5) // 6)           # a pass never leaves its 32-crop block


@pytest.mark.parametrize("n", [N_STEP, N_FITS])
def test_structural_crops_lie_where_the_docstring_says(n):
    rows, prs = rc.pool_rules()
    s, s2, m = rc.indices("S", n), rc.indices("S2", n), rc.indices("M", n)
    empty = lambda idx, c: prs[idx[c], 1] == 0
    # the front image's reach: a pass whose last row is `last` is front while 20 + last + 1 <= 393216
    front = lambda last: V3_ROWS + last + 1 <= REACH_ROWS
    only_front = max(c for c in range(19000, 20000) if front(V3_ROWS * c + V3_ROWS - 1))
    only_back = min(c for c in range(19000, 20000) if not front(V3_ROWS * c))
    assert (only_front, only_back) == (19658, 19660) == (rc.LAST_FRONT, rc.FIRST_BACK)
    blk = only_back // BLOCK
    b0 = blk * BLOCK
    assert blk == 614 and b0 == 19648 and b0 <= only_front and only_back < b0 + BLOCK
    # S: one pass of two runs across the switch
    assert tuple(prs[s[b0]]) == (0, 3) and tuple(prs[s[b0 + 31]]) == (7, 3) and all(empty(s, c) for c in range(b0 + 1, b0 + 31))
    passes = [p for p in rc.listed_passes(prs[s]) if b0 * 10 <= p[0][0] < (b0 + 32) * 10]
    assert passes == [[(b0 * 10, 3), ((b0 + 31) * 10 + 7, 3)]]
    first_row = b0 * V3_ROWS + 0                       # pairs 0 .. 2 read V3 rows -2 .. 7, clipped
    last_row = (b0 + 31) * V3_ROWS + 19                # pairs 7 .. 9 read V3 rows 12 .. 21, clipped
    assert front(first_row) and not front(last_row)
    assert (last_row - first_row + 1) * ROWB < 0xF0000000      # the back image's last row from the pass's first: far inside a resource's reach
    # both one-pixel crops leave most of their staged rows to the image
    assert rows[s[b0], 1] < 8 and rows[s[b0 + 31], 1] < 8
    # S2: a run on each side of the switch, in passes that read image rows (a crop of fewer than 20 own rows)
    for c in list(range(19650, 19659)) + list(range(19660, 19671)):
        assert prs[s2[c], 1] > 0 and rows[s2[c], 1] < V3_ROWS and rc.kinds()[s2[c]] == "synth", c
    assert empty(s2, 19659) and empty(s2, 19649) and tuple(prs[s2[b0]]) == (0, 3)
    in_block = [p for p in rc.listed_passes(prs[s2]) if b0 * 10 <= p[0][0] < (b0 + 32) * 10]
    lasts = [(p[-1][0] + p[-1][1] - 1) // 10 for p in in_block]
    assert sum(c <= only_front for c in lasts) >= 9 and sum(c >= only_back for c in lasts) >= 11
    # a pass straddles the switch itself in S2: its first crop is front-only, its last back-only
    assert any(p[0][0] // 10 <= only_front and (p[-1][0] + p[-1][1] - 1) // 10 >= only_back for p in in_block)
    # 4 GB: the V3 row that straddles byte 2^32 and its crop
    row = (1 << 32) // ROWB
    assert row * ROWB < 1 << 32 < (row + 1) * ROWB and row == 419430 and row // V3_ROWS == 20971
    assert (419420, 419439) == (20971 * V3_ROWS, 20971 * V3_ROWS + 19)
    for idx in (s, s2, m):
        for c in range(20965, 20979):
            assert prs[idx[c], 1] > 0 and rc.kinds()[idx[c]] == "synth", c
        r0, nr = rows[idx[20971]]
        assert 419420 + r0 <= row < 419420 + r0 + nr              # the straddling row is one of the crop's own: computed, and read from V3
    # the workgroups of the pair list: 256 threads x 32 crops
    assert GROUP == 256 * BLOCK
    for g in range(GROUP, n, GROUP):
        for idx in (s, s2, m):
            assert all(prs[idx[c], 1] > 0 for c in range(g - 2, g + 3)), g
    assert [g for g in range(GROUP, n, GROUP)] == [8192, 16384, 24576]
    assert (n + GROUP - 1) // GROUP == 4
    # the batch's edges
    for idx in (s, s2, m):
        assert prs[idx[0], 1] > 0 and prs[idx[n - 1], 1] > 0 and prs[idx[n - 2], 1] > 0 and empty(idx, n - 3)
    # M is N but for the structural positions, where it is S
    at = np.array(sorted(rc.overrides(n)))
    assert np.array_equal(m[at], s[at])
    rest = np.ones(n, bool); rest[at] = False
    assert np.array_equal(m[rest], rc.indices("N", n)[rest])


def test_pool_stays_inside_the_guard_band():
    """every pool crop below limit x (1 - 0.005) at all three stages, by the fp32 oracle: the range guard has nothing to say about any batch"""
    st = weights.synthetic_state(100, 31)
    maxima = cnn_oracle.stage_maxima(st, np.array(rc.pool()), dtype=torch.float32, threads=16)
    noise = rc.kinds() == "noise"
    print("fp32 stage maxima: noise %s, others %s" % ([float(m[noise].max()) for m in maxima], [float(m[~noise].max()) for m in maxima]))
    for m, lim in zip(maxima, rc.LIMITS):
        assert len(m) == 509 and np.all(m < lim * (1 - rc.BAND)), (float(m.max()), lim)


@pytest.mark.parametrize("n", [3200, N_STEP, N_FITS])
def test_the_form_of_conv3_follows_from_the_inputs(n):
    """S and S2: fewer listed passes than the dense kernel's -- the listed form runs; N and M: more -- the dense one.  The passes are counted
    exactly, by the packing restated in cnn_reach_cases.listed_passes.  (The coarse bound ceil(listed / 6) + crops with pairs is printed: it
    exceeds the dense passes wherever most crops list six pairs or more, as the synthetic crops do, and decides nothing there.)"""
    for kind in ("S", "S2", "N", "M"):
        e = rc.expected_stats(kind, n)
        _, prs = rc.pool_rules()
        with_pairs = int((prs[rc.indices(kind, n)][:, 1] > 0).sum())
        coarse = (e["listed"] + 5) // 6 + with_pairs
        print("%s at %d: %d of %d pairs listed, %d listed passes (coarse bound %d) against %d dense; skip %s" %
              (kind, n, e["listed"], e["pairs"], e["list_passes"], coarse, e["dense_passes"], e["skip"]))
        assert (e["listed"] + 5) // 6 <= e["list_passes"] <= coarse
        assert e["dense_passes"] == -(-n * 100 // 64)
        if kind in ("S", "S2"):
            assert e["use_list"] and 0 < e["listed"] < e["pairs"] and e["skip"][1] < e["skip"][0]
            assert e["listed"] < e["dense_passes"] * 6                    # fewer than the dense passes' worth of pairs
        else:
            assert not e["use_list"] and e["list_passes"] >= e["dense_passes"]
        if kind == "N":
            assert e["skip3"] == (10 * n, 10 * n, 0, 0) and e["skip"][1] == e["skip"][0] and e["skip"][2] == 0
        if kind == "M":
            assert e["skip"][1] < e["skip"][0] and e["skip"][2] > 0           # conv2 skips, k_v3_fill copies
