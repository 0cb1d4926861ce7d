"""trexhip_prefilter_device (trex_amd/csrc/prefilter.hip) against tests/prefilter_ref.py, the line-by-line restatement of Tracker::prefilter's
blob policy: d_decision, d_order, d_counts and d_presumed_nr byte for byte, on the hand-worked scenes of tests/prefilter_cases.py
(64 x 48 frames, 2 to 3 per batch, at most 8 blobs per frame)."""
import numpy as np
import pytest
import torch
from oracle import oracle
from trex_amd import capi
import prefilter_cases as pc
import prefilter_ref as ref
from split_cases import merged_scene

pytestmark = pytest.mark.gpu

MAX_BLOBS = 8


def _batch(*scenes):
    return np.stack([pc.paint(s) for s in scenes])


def _context(n, bg, W=pc.W, H=pc.H, max_blobs=MAX_BLOBS):
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=n, max_blobs=max_blobs, cm_per_pixel=1.0))
    seg.set_background(bg)
    return seg


def _load_bodies(seg, bodies):
    off = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int64)
    cat = np.concatenate([np.asarray(b, np.uint8) for b in bodies] + [np.zeros(1, np.uint8)])
    d, o = torch.from_numpy(cat).cuda(), torch.from_numpy(off).cuda()
    seg.load_frames_v6_device(d.data_ptr(), o.data_ptr(), len(bodies), 0)
    return d, o


def device(frames, st, bg=None, load=False, second_count=False, calls=1, max_blobs=MAX_BLOBS):
    """-> det tables, sub tables, [PrefilterResult per call]"""
    bg = pc.background() if bg is None else bg
    n, H, W = frames.shape
    seg = _context(n, bg, W, H, max_blobs)
    d = torch.from_numpy(frames).cuda()
    seg.segment_device(d.data_ptr(), n)
    det = seg.fetch()
    if load:                                                  # the same frames as a stored batch, in a second context
        bodies = [oracle.pv_serialize_v6(r.blobs, r.runs, r.pixels, 0) for r in det]
        seg.close()
        seg = _context(n, bg, W, H, max_blobs)
        keep = _load_bodies(seg, bodies)
        det = seg.fetch()
    pf = capi.Prefilter(seg, n, sum(len(r.blobs) for r in det))
    got = []
    for _ in range(calls):
        pf.run(st.track_threshold, st.method, st.track_size_filter, st.track_threshold_2, st.threshold_ratio_range,
               [s.tolist() for s in st.track_include], [s.tolist() for s in st.track_ignore], st.track_ignore_bdx, second_count=second_count)
        got.append(pf.fetch())
    sub = seg.fetch(rethreshold=True)
    pf.close()
    seg.close()
    return det, sub, got


def check(frames, st, bg=None, max_blobs=MAX_BLOBS, **kw):
    bg = pc.background() if bg is None else bg
    det, sub, got = device(frames, st, bg, max_blobs=max_blobs, **kw)
    want = ref.expected_outputs(det, sub, bg, st, len(frames), max_blobs)
    for g in got:
        for name, w in zip(("decision", "order", "counts", "presumed_nr"), want):
            assert getattr(g, name).tobytes() == w.tobytes(), (name, getattr(g, name), w)
    return det, sub, got, want


ALL = pc.SIZES + pc.DUMBBELL + pc.WEAK                         # 5 detect blobs
CASES = {
    "sizes": (dict(track_threshold=30, track_size_filter=[(20, 100)]), [pc.SIZES, ALL]),
    "split_in_two": (dict(track_threshold=30, track_size_filter=[(20, 100)]), [pc.DUMBBELL, pc.DUMBBELL + pc.SIZES, pc.WEAK]),
    "unthresholded_added": (dict(track_threshold=30), [pc.WEAK, ALL]),
    "empty_filter": (dict(track_threshold=30), [pc.SIZES, pc.SHAPE_BLOBS]),
    "threshold_zero": (dict(track_threshold=0, track_size_filter=[(20, 100)]), [pc.SIZES, ALL]),
    "two_ranges": (dict(track_threshold=30, track_size_filter=[(100, 130), (5, 8)]), [ALL, pc.SIZES]),
    "include_rect": (dict(track_threshold=30, track_include=[[(12, 12), (40, 40)]]), [pc.SHAPE_BLOBS, ALL]),
    "include_rect_edge": (dict(track_threshold=30, track_include=[[(0, 0), (12, 40)]]), [pc.SHAPE_BLOBS, ALL]),
    "ignore_rect": (dict(track_threshold=30, track_ignore=[[(12, 12), (40, 40)]]), [pc.SHAPE_BLOBS, ALL]),
    "include_polygon": (dict(track_threshold=30, track_include=[pc.L_SHAPE]), [pc.SHAPE_BLOBS, ALL]),
    "ignore_polygon": (dict(track_threshold=30, track_ignore=[pc.L_SHAPE, [(50, 0), (64, 48)]]),
                       [pc.SHAPE_BLOBS + [(10, 5, 13, 7, 100), (24, 20, 27, 23, 100)], ALL]),
    "bounds_overlap_centre_outside": (dict(track_threshold=30, track_include=[[(13, 0), (40, 40)]], track_size_filter=[(5, 100)]), [pc.SHAPE_BLOBS, ALL]),
    "include_and_ignore": (dict(track_threshold=30, track_include=[[(0, 0), (40, 48)], pc.L_SHAPE], track_ignore=[[(0, 18), (20, 28)]]), [ALL, pc.SHAPE_BLOBS]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_reference(name):
    kw, scenes = CASES[name]
    det, sub, got, want = check(_batch(*scenes), ref.Settings(**kw))
    assert want[2][:, :3].sum() > 0


@pytest.mark.parametrize("method", [0, 1, 2])
def test_each_difference_method(method):
    # method 2 thresholds the grey value itself: of the values 100 / 160 / 180 on 200 only the weak pixels (180) pass 170
    st = ref.Settings(track_threshold=30 if method < 2 else 170, method=method, track_size_filter=[(20, 100)], track_threshold_2=60 if method < 2 else 175,
                      threshold_ratio_range=(0.5, 2.0))
    det, sub, got, want = check(_batch(ALL, pc.SECOND_IN + pc.SECOND_OUT), st)
    assert want[2][:, 0].sum() > 0


@pytest.mark.parametrize("thr2", [0, 60])
def test_second_threshold_on_and_off(thr2):
    st = ref.Settings(track_threshold=30, track_threshold_2=thr2, threshold_ratio_range=(0.5, 1.0), track_size_filter=[(20, 100)])
    det, sub, got, want = check(_batch(pc.SECOND_IN + pc.SECOND_OUT, pc.SIZES, pc.WEAK), st, second_count=True)
    sec = got[0].second_count
    if thr2 == 0:
        assert (sec == -1).all()                               # k_pre_count2 was not launched: nothing was counted
        assert (want[0] == ref.FILTERED + ref.SECOND_THRESHOLD).sum() == 0
    else:
        counted = want[4] >= 0
        assert counted.sum() == 3 and np.array_equal(sec[counted], want[4][counted])     # 15, 12 and the all-strong blob's 30
        assert (want[0] == ref.FILTERED + ref.SECOND_THRESHOLD).sum() == 2


def test_second_count_of_an_unthresholded_blob():
    # track_threshold 0: nothing is thresholded, the detect blobs themselves reach the second-threshold test (30 pixels, 15 and 12 at 60)
    st = ref.Settings(track_threshold=0, track_threshold_2=60, track_size_filter=[(20, 100)])
    det, sub, got, want = check(_batch(pc.SECOND_IN + pc.SECOND_OUT, pc.SIZES), st, second_count=True)
    counted = want[4] >= 0
    assert sorted(want[4][counted].tolist()) == [12, 15, 30] and (np.nonzero(counted)[0] >= got[0].cap).all()
    assert np.array_equal(got[0].second_count[counted], want[4][counted])
    # nothing survives 30, the second threshold lies below it: the un-thresholded blob has recount 0 and 25 pixels at 10
    st = ref.Settings(track_threshold=30, track_threshold_2=10, track_size_filter=[(0, 100)])
    det, sub, got, want = check(_batch(pc.WEAK, pc.SIZES), st, second_count=True)
    assert got[0].second_count[got[0].cap] == 25 and want[0][got[0].cap] == ref.FILTERED + ref.SECOND_THRESHOLD


def test_bdx_ignored_blobs():
    frames = _batch(pc.SIZES, pc.DUMBBELL)
    det, sub, _ = device(frames, ref.Settings(track_threshold=30))
    a = int(det[0].blobs["bid"][pc.blob_at(det[0], 4, 4)])
    small = int(sub[1].blobs["bid"][pc.blob_at(sub[1], 14, 21)])
    assert small != int(det[1].blobs["bid"][0])
    st = ref.Settings(track_threshold=30, track_size_filter=[(2, 100)], track_ignore_bdx=[{a, 7, 0xFFFFFFFF}, {small}])
    det, sub, got, want = check(frames, st)
    assert (want[0] == ref.FILTERED + ref.BDX_IGNORED).sum() == 2
    # a sub-blob is ignored through its parent's bid as well, and a frame without a list ignores nothing
    st = ref.Settings(track_threshold=30, track_ignore_bdx=[None, {int(det[1].blobs["bid"][0])}])
    check(frames, st)


def test_an_overflowing_frame_beside_a_healthy_one():
    nine = [(2 + 6 * i, 2, 4 + 6 * i, 4, 100) for i in range(9)]            # 9 blobs > max_blobs
    frames = _batch(pc.SIZES, nine, ALL)
    det, sub, got, want = check(frames, ref.Settings(track_threshold=30, track_size_filter=[(20, 100)]))
    assert det[1].info["flags"] != 0 and want[2][:, 3].tolist() == [0, 1, 0] and want[2][0].tolist() == [1, 1, 1, 0]


def _presumed_by_frame(det, got):
    """presumed_nr is in pooled order of the detect table, as the split search reads it; a segmented batch pools its frames in the order
    they finish and a loaded one in frame order, so it is compared frame by frame.  The other outputs are numbered by frame."""
    return [got.presumed_nr[int(d.info["blob_begin"]):int(d.info["blob_begin"]) + len(d.blobs)].tobytes() for d in det]


def test_loaded_batch_equals_segmented_batch():
    st = ref.Settings(track_threshold=30, track_threshold_2=60, track_size_filter=[(20, 100)], track_include=[[(0, 0), (50, 48)]])
    frames = _batch(ALL, pc.SECOND_IN + pc.SECOND_OUT, pc.SHAPE_BLOBS)
    seg_det, seg_sub, seg_got, _ = check(frames, st)
    load_det, load_sub, load_got, _ = check(frames, st, load=True)
    for name in ("decision", "order", "counts"):
        assert getattr(seg_got[0], name).tobytes() == getattr(load_got[0], name).tobytes(), name
    assert _presumed_by_frame(seg_det, seg_got[0]) == _presumed_by_frame(load_det, load_got[0])
    assert sum(len(x) for x in _presumed_by_frame(seg_det, seg_got[0])) == seg_got[0].presumed_nr.nbytes               # every blob compared
    assert (load_got[0].counts[:, :3].sum(axis=1) >= 2).all()                              # every frame decided something


def test_two_consecutive_calls_give_equal_bytes():
    st = ref.Settings(track_threshold=30, track_threshold_2=60, track_size_filter=[(20, 100)], track_ignore=[pc.L_SHAPE])
    det, sub, got, want = check(_batch(ALL, pc.SHAPE_BLOBS + pc.SECOND_IN), st, calls=2, second_count=True)
    for name in ("decision", "order", "counts", "presumed_nr", "second_count"):
        assert getattr(got[0], name).tobytes() == getattr(got[1], name).tobytes(), name


def test_presumed_nr_feeds_the_split_search():
    # merged individuals: the device's presumed_nr handed straight to the split search = the existing route (presumed_nr built on the host
    # from the fetched tables)
    scenes = [merged_scene(50 + s) for s in range(2)]
    frames, bg = np.stack([s[0] for s in scenes]), scenes[0][1]
    n, H, W = frames.shape
    ranges = [(40, 330)]
    st = ref.Settings(track_threshold=16, method=1, track_size_filter=ranges)
    seg = _context(n, bg, W, H, 64)
    d = torch.from_numpy(frames).cuda()
    seg.segment_device(d.data_ptr(), n)
    det = seg.fetch()
    nb = sum(len(r.blobs) for r in det)
    pf = capi.Prefilter(seg, n, nb)
    pf.run(16, 1, ranges)
    got = pf.fetch()
    sub = seg.fetch(rethreshold=True)
    want = ref.expected_outputs(det, sub, bg, st, n, 64)
    assert got.presumed_nr.tobytes() == want[3].tobytes() and (want[3] == 2).sum() >= 2
    thr, info = [], []
    for src in (pf.d_presumed_nr, None):
        d_pres = torch.from_numpy(want[3]).cuda()
        d_thr = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
        d_info = torch.zeros(nb * capi.SPLIT_INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        seg.split_search_device(src if src is not None else d_pres.data_ptr(), nb, d_thr.data_ptr(), d_info.data_ptr(), method=1, size_ranges=ranges,
                                track_threshold=16)
        seg.synchronize()
        thr.append(d_thr.cpu().numpy()); info.append(d_info.cpu().numpy())
    assert np.array_equal(thr[0], thr[1]) and np.array_equal(info[0], info[1]) and (thr[0] >= 0).sum() >= 1
    pf.close()
    seg.close()


def test_refusals():
    frames = _batch(pc.SIZES, pc.SIZES)
    seg = _context(2, pc.background())
    pf = capi.Prefilter(seg, 2, 8)
    with pytest.raises(capi.TrexHipError) as e:               # no batch yet
        pf.run(30)
    assert e.value.code == -1
    d = torch.from_numpy(frames).cuda()
    seg.segment_device(d.data_ptr(), 2)
    with pytest.raises(capi.TrexHipError) as e:               # not fetched
        pf.run(30)
    assert e.value.code == -1
    seg.fetch()
    with pytest.raises(capi.TrexHipError) as e:
        pf.run(30, size_ranges=[(i, i + 1) for i in range(9)])
    assert e.value.code == -4 and "8 ranges" in str(e.value)
    with pytest.raises(capi.TrexHipError) as e:
        pf.run(30, include=[[(i, 0), (i + 1, 1)] for i in range(65)])
    assert e.value.code == -4 and "64 shapes" in str(e.value)
    with pytest.raises(capi.TrexHipError) as e:
        pf.run(30, ignore=[[(i, i) for i in range(4097)]])
    assert e.value.code == -4
    with pytest.raises(capi.TrexHipError) as e:
        pf.run(30, method=3)
    assert e.value.code == -1
    pf.run(30, size_ranges=[(i, i + 1) for i in range(8)], include=[[(i, 0), (i + 1, 1)] for i in range(64)])       # the limits themselves pass
    assert pf.fetch().counts[:, 3].tolist() == [0, 0]
    pf.close()
    seg.close()


def test_run_length_edges_of_the_second_count():
    # k_pre_count2: a 1-pixel line, a 41-pixel line that starts unaligned and crosses 16-byte boundaries, lines ending at the last column
    f = pc.run_edge_frame()
    frames = np.stack([f, f[::-1].copy()])
    st = ref.Settings(track_threshold=30, track_threshold_2=60, threshold_ratio_range=(0.0, 2.0))
    det, sub, got, want = check(frames, st, second_count=True)
    sec = got[0].second_count
    for fi, fr in enumerate(frames):
        strong = (200 - fr.astype(int)) >= 60
        assert len(sub[fi].blobs) == 2
        for k, b in enumerate(sub[fi].blobs):
            runs = sub[fi].runs[b["run_begin"]:b["run_begin"] + b["n_runs"]]
            n = sum(int(strong[r["y"], r["x0"]:r["x1"] + 1].sum()) for r in runs)
            assert n in (13, 4) and sec[fi * MAX_BLOBS + k] == n
    assert {int(r["x1"]) - int(r["x0"]) + 1 for r in sub[0].runs} == {41, 1, 34, 24}
