"""The track-stage re-threshold behind every labelling path of the detect pass.  k_sub does not start from the detect tables trexhip_fetch returns
but from the run-level state the labelling kernels leave in global memory for it alone (row_base, raster, parent, root_ord, blob_map); the detect
tests hold the tables of every path to the oracle and never read that state.  Here every path is followed by a re-threshold whose sub-blob table,
lines and pixels are oracle.rethreshold_frame's bytes (parent counted from the frame's blob_begin).  Pass 2's own overflow: reported, and kept
inside the frame."""
import numpy as np
import pytest
import torch
from oracle import oracle
from trex_amd import capi, synth
import ccl_scenes as cs
from rethreshold_checks import assert_per_blob_equal, assert_sub_equal, rebased

pytestmark = pytest.mark.gpu


def context(bg, max_batch, **caps):
    H, W = bg.shape
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=max_batch, **caps))
    seg.set_background(bg)
    return seg


def detect(seg, frames):
    """segment + fetch -> the detect FrameResults and the device tensor the context goes on reading"""
    d = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.stack(frames))).cuda()
    seg.segment_device(d.data_ptr(), len(d))
    return seg.fetch(), d


def rethreshold(seg, thr, method, ranges=()):
    seg.rethreshold(thr, method, ranges)
    return seg.fetch(rethreshold=True)


def same_tables(a, b):
    return len(a) == len(b) and all(x.blobs.tobytes() == y.blobs.tobytes() and x.runs.tobytes() == y.runs.tobytes() and x.pixels.tobytes() == y.pixels.tobytes()
                                    and x.info.tobytes() == y.info.tobytes() for x, y in zip(a, b))


def assert_batch(det, sub, batch, key_of, ranges, method, thr, **detect_kw):
    """batch[i] names the distinct frame in slot i: its first instance against the oracle, its other copies against that instance's bytes"""
    first = {}
    for i, k in enumerate(batch):
        if k not in first:
            first[k] = i
            assert_sub_equal(sub[i], det[i], cs.sub_tables(key_of(k), method, thr, ranges, **detect_kw))
        else:
            assert sub[i].info["flags"] == 0
            assert rebased(sub[i], det[i]) == rebased(sub[first[k]], det[first[k]]), (i, k, method, thr)


def test_behind_the_s_m_and_l_instances_by_the_shipped_policy():
    """The batch sequence of test_instance_ladder_by_the_shipped_policy (test_segment_gpu.py) on the textured ladder, two frames per CU, gather fused
    into k_ccl_lds: all light (S), medium frames in the first, a middle and the last slot (S, the medium ones finished by the L retry; then M), heavy
    frames beside them (M, the heavy ones finished by the L retry; then L).  Which instance ran follows from launch_segment's code and the line counts
    asserted here, as in the detect test; it is not observed.  After every call: fetch, and at each (method, threshold) re-threshold and fetch.  This is
    the only reader of what phases P5-P7 of the S and M instances and of the retry store into raster, parent, root_ord and blob_map."""
    cs.check_ladder()
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    bg, distinct = cs.textured_ladder()
    all_light = [i % 2 for i in range(n)]                            # indices into `distinct`
    with_medium = list(all_light); with_medium[0] = 2; with_medium[n // 2] = 3; with_medium[n - 1] = 2
    with_heavy = list(with_medium); with_heavy[1] = 4; with_heavy[n // 2 + 1] = 5; with_heavy[n - 2] = 4
    seg = context(bg, n, **cs.LADDER_CAPS)
    pool = torch.from_numpy(np.stack(distinct)).cuda()
    tables = []
    for batch in (all_light, with_medium, with_medium, with_heavy, with_heavy):
        d = pool[torch.tensor(batch, device="cuda")].contiguous()
        det, _ = detect(seg, d)
        for i, k in enumerate(batch):
            lo, hi = cs.LADDER_BRACKET[k]
            assert det[i].info["flags"] == 0 and lo <= det[i].info["n_raw_runs"] <= hi, (i, k)
        sig = []
        for method, thr in cs.TRACK_PAIRS:
            sub = rethreshold(seg, thr, method, cs.TRACK_RANGES)
            assert_batch(det, sub, batch, lambda k: ("ladder", k), cs.TRACK_RANGES, method, thr)
            sig.append([rebased(s, dd) for s, dd in zip(sub, det)])
        tables.append(sig)
    seg.close()
    assert tables[1] == tables[2] and tables[3] == tables[4]


@pytest.fixture(scope="module")
def band_scenes():
    bg, frames = cs.textured_band_frames()
    keys = [cs.register(("band", i), bg, f) for i, f in enumerate(frames)]
    for conn in (8, 4):
        for k in keys[:-1]:
            cs.check_capacities(k, cs.BAND_CAPS, connectivity=conn)
    assert len(cs.detect_tables(keys[-1])[1]) == 0                    # the empty frame
    obg, of = cs.odd_height_frame()
    cs.check_capacities(cs.register("odd_height", obg, of), cs.BAND_CAPS)
    return bg, frames, keys, obg, of


@pytest.mark.parametrize("bands", [2, 3, 8])
def test_behind_band_workgroups(bands, band_scenes, monkeypatch):
    """k_ccl_band + the seam-linking k_ccl_lds, forced (TREXHIP_CCL_BANDS): the scenes of test_several_workgroups_per_frame_give_the_same_tables,
    textured -- blobs through every seam, a bar on the middle seam, a frame whose band overflows its band workgroup (labelled by the one workgroup
    after all), an empty frame -- at 8- and 4-connectivity (k_link2's c.slack), and an odd height whose last band is shorter.  The only reader of the
    raster / parent / root_ord / blob_map that k_ccl_lds leaves after reloading the bands' labels."""
    monkeypatch.setenv("TREXHIP_CCL_BANDS", str(bands))
    bg, frames, keys, obg, of = band_scenes
    d = torch.from_numpy(np.stack(frames)).cuda()
    for conn in (8, 4):
        seg = context(bg, len(frames), connectivity=conn, **cs.BAND_CAPS)
        det, _ = detect(seg, d)
        for method, thr in cs.TRACK_PAIRS:
            sub = rethreshold(seg, thr, method, cs.TRACK_RANGES)
            for i, k in enumerate(keys):
                assert_sub_equal(sub[i], det[i], cs.sub_tables(k, method, thr, cs.TRACK_RANGES, connectivity=conn))
        seg.close()
    seg = context(obg, 1, **cs.BAND_CAPS)
    det, _d = detect(seg, [of])
    for method, thr in cs.TRACK_PAIRS:
        assert_sub_equal(rethreshold(seg, thr, method, cs.TRACK_RANGES)[0], det[0], cs.sub_tables("odd_height", method, thr, cs.TRACK_RANGES))
    seg.close()


def test_behind_the_global_memory_chain():
    """One batch: a frame of more than 8160 lines (launch_pending: k_rowscan, k_link, k_flatten, k_blobs in global memory), a frame k_ccl_lds labels
    and an empty one.  The pending frame's run-level state has to be right and the finished frames' state untouched by the chain: the only reader
    of what k_link / k_flatten / k_blobs (only_pending) leave in parent, root_ord and blob_map."""
    bg, frames = cs.global_chain_frames()
    keys = [cs.register(("chain", i), bg, f) for i, f in enumerate(frames)]
    for k in keys[:2]:
        cs.check_capacities(k, cs.BAND_CAPS)
    assert len(cs.detect_tables(keys[0])[1]) > cs.CCL_NMAX >= len(cs.detect_tables(keys[1])[1]) > 0 == len(cs.detect_tables(keys[2])[1])
    seg = context(bg, 3, **cs.BAND_CAPS)
    det, _d = detect(seg, frames)
    assert det[0].info["n_raw_runs"] > cs.CCL_NMAX
    for method, thr in cs.TRACK_PAIRS:
        sub = rethreshold(seg, thr, method, cs.TRACK_RANGES)
        for i, k in enumerate(keys):
            assert_sub_equal(sub[i], det[i], cs.sub_tables(k, method, thr, cs.TRACK_RANGES))
    seg.close()


def test_behind_the_l_instance_with_a_separate_gather():
    """Just under 3/4 of a frame per CU: the L instance of k_ccl_lds labels every frame and k_gather runs as its own launch (at 3/4 and above it is
    fused into k_ccl_lds), many frames, light and medium.  The only reader of the L instance's run-level stores at a frame count beyond a handful."""
    cs.check_ladder()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (3 * cus - 1) // 4
    assert n >= 4 and 4 * n < 3 * cus
    bg, distinct = cs.textured_ladder()
    batch = [(i * 7 + i // 5) % 4 for i in range(n)]                 # noise and structured, light and medium, in no regular order
    seg = context(bg, n, **cs.LADDER_CAPS)
    det, _d = detect(seg, [distinct[k] for k in batch])
    for method, thr in cs.TRACK_PAIRS:
        sub = rethreshold(seg, thr, method, cs.TRACK_RANGES)
        assert_batch(det, sub, batch, lambda k: ("ladder", k), cs.TRACK_RANGES, method, thr)
    seg.close()


@pytest.mark.parametrize("method", [0, 1])
def test_per_blob_thresholds_on_heavy_frames(method):
    """rethreshold_per_blob on a medium and a heavy structured frame (a few blobs of thousands of lines each: one threshold governs thousands of k_sub's
    threads) and a noise frame of hundreds of blobs; every fifth blob is left out.  Per detect blob against oracle.threshold_blob."""
    thresholds, ranges = cs.check_per_blob_scene(method)
    bg, distinct = cs.textured_ladder()
    frames = [distinct[k] for k in cs.PER_BLOB_FRAMES]
    seg = context(bg, len(frames), **cs.LADDER_CAPS)
    det, _d = detect(seg, frames)
    pooled = np.full(sum(len(r.blobs) for r in det), -1, np.int32)   # pooled order: a frame's blobs start at its blob_begin
    for r, thr in zip(det, thresholds):
        assert len(r.blobs) == len(thr)
        pooled[int(r.info["blob_begin"]):int(r.info["blob_begin"]) + len(thr)] = thr
    dthr = torch.from_numpy(pooled).cuda()
    seg.rethreshold_per_blob(dthr.data_ptr(), method=method, size_ranges=ranges)
    sub = seg.fetch(rethreshold=True)
    for r, s, thr in zip(det, sub, thresholds):
        assert_per_blob_equal(r, s, bg, thr, method, ranges)
    seg.close()


# ---- pass 2's own overflow ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", [1, 3])
def test_pass2_run_overflow_is_reported_and_stays_inside_the_frame(slot):
    """A line of L pixels breaks into up to ceil(L / 2) sub-runs, so a frame whose detect lines fit max_runs can have more sub-runs than that
    (here 56 lines, 6720 sub-runs, max_runs 4096).  k_sub_scan flags the frame; the emitting k_sub has to leave it alone, or its stores land in the
    next frame's share of raster2 / run_parent2 (slot 1) or behind the last frame's (slot 3: the context is created with one frame more than it is
    handed, so that even then the memory is the context's own).  A spill into the neighbour RACES with the neighbour's own stores of the same
    launch, so a wrong kernel need not fail here: this test pins what is reported and the neighbours' tables; that the guard holds is argued from
    k_sub's code (it returns for a frame whose info2 carries a flag, and a frame without one has n2 <= max_runs)."""
    cs.check_pass2_overflow()
    obg, of = cs.pass2_overflow_frame()
    H, W = obg.shape
    rng = np.random.default_rng(slot)
    others = []
    for _ in range(3):                                               # ordinary frames: a few textured blocks each
        f = obg.copy()
        for j in range(6):
            y, x = int(rng.integers(0, H - 10)), int(rng.integers(0, W - 30))
            f[y:y + 9, x:x + 28] = rng.integers(1, 150, (9, 28))
        others.append(f)
    frames = others[:slot] + [of] + others[slot:]
    keys = [cs.register(("pass2_overflow_batch", slot, i), obg, f) for i, f in enumerate(frames)]
    caps = dict(max_runs=cs.OVERFLOW_MAX_RUNS, max_blobs=4096, max_pixels=W * H)
    for i, k in enumerate(keys):
        if i != slot:
            cs.check_capacities(k, caps, pairs=((0, 150), (0, 60)), ranges=())
    seg = context(obg, len(frames) + 1, **caps)
    det, _d = detect(seg, frames)
    assert all(r.info["flags"] == 0 for r in det) and det[slot].info["n_raw_runs"] == 56
    seg.last_capacity_error = None
    sub = rethreshold(seg, 150, 0)
    assert seg.last_capacity_error                                   # trexhip_fetch_rethreshold returned TREXHIP_E_CAPACITY
    for i, k in enumerate(keys):
        if i == slot:
            assert sub[i].info["flags"] == capi.FRAME_OVERFLOW_RUNS and len(sub[i].blobs) == 0 and len(sub[i].runs) == 0
            assert sub[i].info["n_raw_runs"] == 6720
        else:
            assert_sub_equal(sub[i], det[i], cs.sub_tables(k, 0, 150))
    assert same_tables(seg.fetch(), det)                             # the detect tables are what they were
    seg.last_capacity_error = None
    sub = rethreshold(seg, 60, 0)                                    # the same batch at a threshold that fits
    assert seg.last_capacity_error is None
    for i, k in enumerate(keys):
        assert_sub_equal(sub[i], det[i], cs.sub_tables(k, 0, 60))
    det, _d = detect(seg, [obg] * len(frames))                       # ... and the context is clean for the next batch
    sub = rethreshold(seg, 150, 0)
    assert all(r.info["flags"] == 0 and len(r.blobs) == 0 for r in det + sub)
    seg.close()


def test_a_frame_that_overflowed_in_the_detect_pass_carries_its_flag_through():
    """frame 0 has more lines than max_runs (as in test_capacity_overflow_is_reported): no detect blobs, the flag; pass 2 copies the flag and
    re-thresholds the other frames as if it were not there"""
    H, W = 64, 256
    bg = np.full((H, W), 200, np.uint8)
    over = bg.copy(); over[:, ::2] = 5                               # 128 lines per row, 8192 in all
    rng = np.random.default_rng(9)
    frames = [over]
    for _ in range(2):
        f = bg.copy()
        for j in range(6):
            y, x = int(rng.integers(0, H - 10)), int(rng.integers(0, W - 30))
            f[y:y + 9, x:x + 28] = rng.integers(1, 150, (9, 28))
        frames.append(f)
    keys = [cs.register(("detect_overflow_batch", i), bg, f) for i, f in enumerate(frames)]
    caps = dict(max_runs=1000, max_blobs=4096, max_pixels=W * H)
    assert len(cs.detect_tables(keys[0])[1]) == 8192 > caps["max_runs"]
    for k in keys[1:]:
        cs.check_capacities(k, caps, pairs=((0, 100),), ranges=cs.TRACK_RANGES)
    seg = context(bg, len(frames), **caps)
    det, _d = detect(seg, frames)
    assert det[0].info["flags"] & capi.FRAME_OVERFLOW_RUNS and [int(r.info["flags"]) for r in det[1:]] == [0, 0]
    sub = rethreshold(seg, 100, 0, cs.TRACK_RANGES)
    assert sub[0].info["flags"] == det[0].info["flags"] and len(sub[0].blobs) == 0
    for i in (1, 2):
        assert_sub_equal(sub[i], det[i], cs.sub_tables(keys[i], 0, 100, cs.TRACK_RANGES))
    seg.close()


def test_pass2_blob_overflow_is_reported_alone():
    """eight detect blobs, 2304 one-pixel survivors at threshold 150 against max_blobs = 512: the detect pass fits, every run count fits, pass 2
    reports TREXHIP_FRAME_OVERFLOW_OUTPUT and nothing else for that frame, and its neighbour is the oracle's"""
    cs.check_pass2_many_blobs()
    bg, f = cs.pass2_many_blobs_frame()
    H, W = bg.shape
    plain = bg.copy(); plain[10:40, 20:200] = np.random.default_rng(3).integers(1, 150, (30, 180))
    key = cs.register("pass2_many_blobs_neighbour", bg, plain)
    caps = dict(max_runs=8000, max_blobs=cs.MANY_BLOBS_MAX_BLOBS, max_pixels=W * H)
    cs.check_capacities(key, caps, pairs=((0, 150),), ranges=())
    seg = context(bg, 2, **caps)
    det, _d = detect(seg, [f, plain])
    assert det[0].info["flags"] == 0 and len(det[0].blobs) == 8
    seg.last_capacity_error = None
    sub = rethreshold(seg, 150, 0)
    assert seg.last_capacity_error
    assert sub[0].info["flags"] == capi.FRAME_OVERFLOW_OUTPUT and len(sub[0].blobs) == 0
    assert_sub_equal(sub[1], det[1], cs.sub_tables(key, 0, 150))
    seg.close()
