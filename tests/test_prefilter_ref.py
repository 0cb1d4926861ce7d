"""Hand-worked cases for tests/prefilter_ref.py, the restatement of Tracker::prefilter's blob policy (Tracker.cpp:742-914) that the device
call is held to: each scene is small enough to check on paper (tests/prefilter_cases.py).  Tables come from the CPU oracle."""
import numpy as np
import pytest
from oracle import oracle
import prefilter_cases as pc
import prefilter_ref as ref
from prefilter_ref import COMMITTED, BIG, FILTERED, NONE


class Table:
    def __init__(self, t):
        self.blobs, self.runs, self.pixels = t
        self.info = {"flags": 0, "blob_begin": 0}


def tables(frame, track_threshold, method=0):
    bg = pc.background()
    p = oracle.make_params(pc.W, pc.H)
    return Table(oracle.segment(frame, bg, p)), Table(oracle.rethreshold_frame(frame, bg, p, method, track_threshold)), bg


def decide(rects, **kw):
    st = ref.Settings(**kw)
    det, sub, bg = tables(pc.paint(rects), st.track_threshold, st.method)
    return det, sub, ref.prefilter_frame(det, sub, bg, st)


def test_inside_below_and_above_the_size_range():
    det, sub, r = decide(pc.SIZES, track_threshold=30, track_size_filter=[(20, 100)])
    a, b, c = pc.blob_at(det, 4, 4), pc.blob_at(det, 20, 4), pc.blob_at(det, 30, 4)
    sa, sc = pc.blob_at(sub, 4, 4), pc.blob_at(sub, 30, 4)
    assert r.det[a] == NONE and r.sub[sa] == COMMITTED                       # 30 px in [20, 100)
    assert r.det[b] == FILTERED + ref.OUTSIDE_RANGE                          # gate shut (4 < 10): the blob itself, 4 < 20
    assert r.sub[pc.blob_at(sub, 20, 4)] == NONE
    assert r.det[c] == NONE and r.sub[sc] == BIG                             # 120 px: neither in range nor below it
    assert r.filtered == [("sub", sa)] and r.big == [("sub", sc)] and r.filtered_out == 1
    assert r.presumed.tolist() == [2 if k == c else 0 for k in range(3)]


def test_a_blob_that_thresholds_into_two():
    det, sub, r = decide(pc.DUMBBELL, track_threshold=30, track_size_filter=[(20, 100)])
    assert len(det.blobs) == 1 and len(sub.blobs) == 2                       # recount 36 >= 10 opens the gate
    big, small = pc.blob_at(sub, 4, 20), pc.blob_at(sub, 14, 21)
    assert r.det[0] == NONE and r.sub[big] == COMMITTED and r.sub[small] == FILTERED + ref.OUTSIDE_RANGE
    assert r.filtered == [("sub", big)] and r.big == [] and r.filtered_out == 1 and r.presumed.tolist() == [0]
    # the small half's own bid on the ignore list: BdxIgnored in the precise check, the other half stays
    det, sub, r = decide(pc.DUMBBELL, track_threshold=30, track_size_filter=[(20, 100)], track_ignore_bdx=[{int(sub.blobs["bid"][small])}])
    assert r.sub[small] == FILTERED + ref.BDX_IGNORED and r.sub[big] == COMMITTED


def test_nothing_survives_so_the_unthresholded_blob_is_added():
    # no size filter (an empty track_size_filter accepts every size): the gate is open, threshold_blob returns nothing
    det, sub, r = decide(pc.WEAK, track_threshold=30)
    assert len(det.blobs) == 1 and len(sub.blobs) == 0
    assert r.det[0] == COMMITTED and r.filtered == [("det", 0)]
    # with a filter its recount is 0: gate shut, 0 < 20 -> OutsideRange
    det, sub, r = decide(pc.WEAK, track_threshold=30, track_size_filter=[(20, 100)])
    assert r.det[0] == FILTERED + ref.OUTSIDE_RANGE and r.filtered == []


def test_empty_size_filter_commits_every_size():
    det, sub, r = decide(pc.SIZES, track_threshold=30)
    assert (r.det == NONE).all() and (r.sub == COMMITTED).all() and len(r.filtered) == 3 and r.big == []
    # track_threshold 0: nothing goes through threshold_blob (Tracker.cpp:830), the blobs themselves are committed
    det, sub, r = decide(pc.SIZES, track_threshold=0)
    assert (r.det == COMMITTED).all() and (r.sub == NONE).all()


def test_second_threshold_ratio_in_and_out():
    kw = dict(track_threshold=30, track_threshold_2=60, threshold_ratio_range=(0.5, 1.0), track_size_filter=[(20, 100)])
    det, sub, r = decide(pc.SECOND_IN + pc.SECOND_OUT, **kw)
    i, o = pc.blob_at(sub, 4, 30), pc.blob_at(sub, 20, 30)
    assert r.second == {("sub", i): 15, ("sub", o): 12}
    assert r.sub[i] == COMMITTED                                             # 15 in [15, 30)
    assert r.sub[o] == FILTERED + ref.SECOND_THRESHOLD                       # 12 < 15
    # all pixels strong: second count = recount = 30, outside [15, 30)
    det, sub, r = decide([pc.SIZES[0]], **kw)
    assert r.sub[0] == FILTERED + ref.SECOND_THRESHOLD and r.second == {("sub", 0): 30}


def test_rectangle_and_concave_polygon_with_the_centre_on_an_edge():
    kw = dict(track_threshold=30)
    sq, lo = (10, 10), (10, 30)

    def at(r, sub, xy):
        return r.sub[pc.blob_at(sub, *xy)]
    # rectangle: the left / top edge belongs to it, the right / bottom edge does not (centre of the square = (12, 12))
    det, sub, r = decide(pc.SHAPE_BLOBS, track_include=[[(12, 12), (40, 40)]], **kw)
    assert at(r, sub, sq) == COMMITTED and at(r, sub, lo) == COMMITTED
    det, sub, r = decide(pc.SHAPE_BLOBS, track_include=[[(0, 0), (12, 40)]], **kw)
    assert at(r, sub, sq) == FILTERED + ref.OUTSIDE_INCLUDE
    det, sub, r = decide(pc.SHAPE_BLOBS, track_ignore=[[(12, 12), (40, 40)]], **kw)
    assert at(r, sub, sq) == FILTERED + ref.INSIDE_IGNORE and at(r, sub, (2, 40)) == COMMITTED
    # concave polygon: (12, 12) lies on its edge y = 12 and counts as outside (two crossings to the right); (12, 31.5) lies in the notch
    det, sub, r = decide(pc.SHAPE_BLOBS, track_include=[pc.L_SHAPE], **kw)
    assert at(r, sub, sq) == FILTERED + ref.OUTSIDE_INCLUDE and at(r, sub, lo) == FILTERED + ref.OUTSIDE_INCLUDE
    det, sub, r = decide(pc.SHAPE_BLOBS + [(10, 5, 13, 7, 100), (24, 20, 27, 23, 100)], track_ignore=[pc.L_SHAPE], **kw)
    assert at(r, sub, (10, 5)) == FILTERED + ref.INSIDE_IGNORE               # centre (12, 6.5): in the horizontal arm
    assert at(r, sub, (24, 20)) == FILTERED + ref.INSIDE_IGNORE              # centre (26, 22): in the vertical arm
    assert at(r, sub, sq) == COMMITTED and at(r, sub, lo) == COMMITTED
    assert ref.pnpoly(np.asarray(pc.L_SHAPE, np.float32), np.float32(12), np.float32(11.5))


def test_bounds_overlap_the_include_rectangle_but_the_centre_is_outside():
    det, sub, r = decide(pc.SHAPE_BLOBS, track_threshold=30, track_include=[[(13, 0), (40, 40)]])
    a, far = pc.blob_at(det, 10, 10), pc.blob_at(det, 2, 40)
    assert r.det[a] == NONE and r.sub[pc.blob_at(sub, 10, 10)] == FILTERED + ref.OUTSIDE_INCLUDE   # bounds reach x = 14, centre 12 < 13
    assert r.det[far] == FILTERED + ref.OUTSIDE_INCLUDE and r.sub[pc.blob_at(sub, 2, 40)] == NONE  # bounds end at x = 6: imprecise check
    assert r.filtered == [] and r.filtered_out == 3


def test_a_bdx_ignored_blob():
    det, sub, _ = decide(pc.SIZES, track_threshold=30)
    a = pc.blob_at(det, 4, 4)
    det, sub, r = decide(pc.SIZES, track_threshold=30, track_ignore_bdx=[{int(det.blobs["bid"][a])}])
    assert r.det[a] == FILTERED + ref.BDX_IGNORED and r.sub[pc.blob_at(sub, 4, 4)] == NONE
    assert len(r.filtered) == 2 and r.filtered_out == 1


def test_expected_outputs_layout():
    st = ref.Settings(track_threshold=30, track_size_filter=[(20, 100)])
    det, sub, bg = tables(pc.paint(pc.SIZES), 30)
    sub.info["blob_begin"] = 0
    decision, order, counts, presumed, second = ref.expected_outputs([det], [sub], bg, st, max_batch=2, max_blobs=8)
    cap = 16
    assert decision.shape == (32,) and order.shape == (1, 16) and counts.tolist() == [[1, 1, 1, 0]]
    assert order[0, :2].tolist() == [pc.blob_at(sub, 4, 4), pc.blob_at(sub, 30, 4)] and (order[0, 2:] == -1).all()
    assert decision[cap + pc.blob_at(det, 20, 4)] == FILTERED + ref.OUTSIDE_RANGE and (second == -1).all()
