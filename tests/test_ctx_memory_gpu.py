"""The context's memory plumbing (trexhip::Mem, Scratch, BlobTables in trex_amd/csrc/internal.h) where it can go wrong: a scratch buffer
that grows, is reused after it grew, or is shared by two entry points; the two table sets fetched in turn; the network's per-batch
buffers growing.  Every case runs its call sequence on one small context (64 x 64 frames, max_batch 4) and compares every result,
byte for byte, with the restatement the entry point's own test uses -- so a buffer of the wrong size, a stale pointer or a size in the
wrong unit shows as a wrong byte, in the call after the growth as much as in the growing one."""
import numpy as np
import pytest
import torch

import augment_ref
import test_averages_gpu as TA
import test_validation_gpu as TV
import uniqueness_ref as U
import visual_field_scenes as S
from oracle import oracle
from trex_amd import capi, weights

pytestmark = pytest.mark.gpu
F = np.float32
W = H = 64
MP = 512


def make_ctx(max_batch=4):
    return capi.Segmenter(capi.default_params(W, H, max_batch=max_batch))


@pytest.fixture(scope="module")
def seg():
    s = make_ctx()
    yield s
    s.close()


def scene64(counts, seed):
    """frames of 64 x 64 on a flat background, counts[f] individuals in frame f, one per 32 x 32 cell so that each is a blob of its own: graded
    ellipses of 12 x 4 px semi-axes, every third one speckled, so that thresholds break it up (kinds 1 and 3 of
    test_posture_gpu._retry_scene at half the size)"""
    rng = np.random.default_rng(seed)
    bg = np.full((H, W), 200, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = []
    for cnt in counts:
        assert cnt <= 4
        fr = bg.astype(np.int32).copy()
        for k in range(cnt):
            cx, cy = 16 + 32 * (k % 2) + rng.integers(-2, 3), 16 + 32 * (k // 2) + rng.integers(-2, 3)
            th = rng.uniform(0, np.pi)
            u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th); v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
            if k % 3 == 2:
                m = (u / 12) ** 2 + (v / 5) ** 2 <= 1
                fr[m] = 200 - rng.integers(16, 120, m.sum())
            else:
                d = (u / 12) ** 2 + (v / 4) ** 2
                m = d <= 1
                fr[m] = (200 - (20 + 120 * (1 - d[m]))).astype(np.int32)
        frames.append(np.clip(fr, 0, 255).astype(np.uint8))
    return np.stack(frames), bg


def segment(seg, fr, bg):
    """segment + fetch; the tables must be the oracle's"""
    seg.set_background(bg)
    seg.frames_alive = d = torch.from_numpy(fr).cuda()        # the context reads the caller's frames again (re-threshold, crops): keep them
    seg.segment_device(d.data_ptr(), len(fr))
    res = seg.fetch()
    same_tables(res, [oracle.segment(f, bg, oracle.make_params(W, H)) for f in fr])
    return res


def same_tables(res, want):
    assert len(res) == len(want)
    for r, (ob, orr, opx) in zip(res, want):
        assert r.blobs.tobytes() == ob.tobytes() and r.runs.tobytes() == orr.tobytes() and r.pixels.tobytes() == opx.tobytes()


# ---- grow, then reuse what grew -----------------------------------------------------------------------------------------------------------
def test_class_averages_small_large_small(seg):
    classes, n_ids = 3, 3
    for n in (4, 300, 4):
        rng = np.random.default_rng([n, classes])
        probs = TA.make_probs(n, classes, rng)
        keys = TA.make_keys("random", n, n_ids, rng)
        d_probs, d_keys = torch.from_numpy(probs).cuda(), torch.from_numpy(keys).cuda()
        got = TA.call(seg, d_probs.data_ptr(), n, classes, d_keys.data_ptr(), n_ids)
        for name, g, w in zip(("samples", "values", "max_index", "max_p"), got, TA.want_bytes(probs, keys, n_ids)):
            assert g == w, (n, name)


def metrics_bytes(m):
    return dict(confusion=m.confusion.tobytes(), accuracy=m.per_class_accuracy.tobytes(), unique_percent=m.unique_percent.tobytes(),
                unique_percent_raw=m.unique_percent_raw.tobytes(), uniqueness_per_class=m.uniqueness_per_class.tobytes(),
                frames=(m.good_frames, m.bad_frames), means=np.array([m.good_ratio, m.mean_unique, m.mean_unique_raw], F).tobytes())


def test_validation_metrics_small_large_small(seg):
    classes = 5
    rows, targets, _ = TV.make_case(classes, 257)            # the special rows (zeros, NaN, ties, denormals) lead
    assert len(rows) >= 400
    small = (6, np.array([(0, 6)], np.int32))
    large = (400, np.array([(10 * k, 10 * k + 10) for k in range(40)], np.int32))
    first = None
    for n, ranges in (small, large, small):
        d_rows, d_targets = torch.from_numpy(rows[:n].copy()).cuda(), torch.from_numpy(targets[:n].copy()).cuda()
        m = seg.validation_metrics(d_rows.data_ptr(), n, classes, d_targets_ptr=d_targets.data_ptr(), frame_ranges=ranges)
        with np.errstate(invalid="ignore"):
            want = U.calculate_uniqueness(rows[:n], [tuple(int(v) for v in r) for r in ranges])
            conf = U.confusion(rows[:n], targets[:n], classes)
            acc = U.per_class_accuracy(rows[:n], targets[:n], classes)
        got = metrics_bytes(m)
        d = np.abs(m.unique_percent.astype(np.float64) - want["unique_percent"].astype(np.float64)).max()
        print(f"n {n}, {len(ranges)} ranges: max |unique_percent - ref| = {d:.3g}; means {m.good_ratio!r} {m.mean_unique!r} {m.mean_unique_raw!r} "
              f"want {want['good_ratio']!r} {want['mean_unique']!r} {want['mean_unique_raw']!r}")
        assert got["confusion"] == conf.tobytes() and got["accuracy"] == acc.tobytes()
        assert got["frames"] == (want["good_frames"], want["bad_frames"])
        assert got["unique_percent_raw"] == want["unique_percent_raw"].tobytes()
        assert got["unique_percent"] == want["unique_percent"].tobytes()
        assert got["uniqueness_per_class"] == want["uniqueness_per_class"].astype(F).tobytes()
        assert got["means"] == np.array([want["good_ratio"], want["mean_unique"], want["mean_unique_raw"]], F).tobytes()
        if first is None:
            first = got
    assert got == first, "the first call's results changed after the buffer grew"


def test_augment_index_list_small_large_small(seg):
    # the index list lives in a buffer of at least 1024 entries: 1500 makes it grow
    pool = augment_ref.sample_images(16, 8, 8, 1, seed=11)
    targets = np.arange(16, dtype=np.int32) * 3 + 1
    d_pool, d_t = torch.from_numpy(pool).cuda(), torch.from_numpy(targets).cuda()
    for n in (8, 1500, 8):
        idx = np.random.default_rng(n).integers(0, 16, n).astype(np.int32)
        d_out = torch.full((n, 8, 8, 1), -7.0, dtype=torch.float32, device="cuda")
        d_to = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        seg.augment_device(d_pool.data_ptr(), 16, n, 8, 8, 1, d_out.data_ptr(), ap=None, indices=idx, d_pool_targets_ptr=d_t.data_ptr(),
                           d_targets_out_ptr=d_to.data_ptr())
        seg.synchronize()
        assert d_out.cpu().numpy().tobytes() == augment_ref.plain(pool[idx]).tobytes(), n
        assert np.array_equal(d_to.cpu().numpy(), targets[idx]), n


def vf_scene(counts, observers, max_points, max_tess, seed):
    """random_frames of the visual-field tests with outline rows of max_points points (every outline must fit) and its own max_tess_points"""
    sc = S.random_frames(seed, counts, observers, specials=False)
    sc.max_tess = max_tess
    a = sc.arrays()
    assert a["info"]["n_outline"].max() <= max_points, f"seed {seed}: an outline of {a['info']['n_outline'].max()} points -- move the seed"
    a["outline"] = np.ascontiguousarray(a["outline"][:, :max_points])
    a["max_points"] = max_points
    rep = {}
    want = S.reference(a, rep)
    assert rep["fragile"] == [], f"seed {seed}: fragile records -- move the seed"
    return a, want


def test_visual_field_small_large_small(seg):
    small = vf_scene([2], [1], 64, 64, 48)                     # max_tess_points may not be below max_points: rows of 64 points
    large = vf_scene([4, 4, 4], [2, 2, 2], S.MAXP, 1024, 43)
    assert (small[1]["status"] == 0).all() and (large[1]["status"] == 0).all()
    for a, want in (small, large, small):
        got = seg.visual_field(a["outline"], a["info"], a["frame_entries"], a["entries"], a["observers"], a["max_points"],
                               max_tess_points=a["max_tess"], max_d=a["max_d"], max_distance=a["max_distance"])
        for k in ("depth", "ids", "points", "fov", "head_distance", "status"):
            g, w = getattr(got, k), want[k]
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (k, a["max_tess"])


def posture_auto(seg, n, tpt=15):
    outline = torch.zeros((n, MP, 2), dtype=torch.float32, device="cuda"); segs = torch.zeros((n, MP // 2 + 1, 4), dtype=torch.float32, device="cuda")
    info = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    thr = torch.zeros(n, dtype=torch.int32, device="cuda"); its = torch.zeros(n, dtype=torch.int32, device="cuda")
    seg.posture_auto_device(n, outline.data_ptr(), segs.data_ptr(), info.data_ptr(), method=0, track_posture_threshold=tpt,
                            d_threshold_ptr=thr.data_ptr(), d_iterations_ptr=its.data_ptr(), max_points=MP)
    seg.synchronize()
    return (info.cpu().numpy().view(capi.POSTURE_INFO_DTYPE).reshape(-1), outline.cpu().numpy(), segs.cpu().numpy(), thr.cpu().numpy(), its.cpu().numpy())


def test_posture_auto_one_blob_all_blobs_one_blob(seg):
    fr, bg = scene64([4, 3, 4, 2], 7)
    res = segment(seg, fr, bg)
    total = sum(len(r.blobs) for r in res)
    assert total == 13
    pp = oracle.posture_params(max_points=MP)
    want = [None] * total                                    # by pooled index: the frames reserve their part of the pool in no fixed order
    for r in res:
        for k, b in enumerate(r.blobs):
            rs = r.runs[b["run_begin"]:b["run_begin"] + b["n_runs"]]; px = r.pixels[b["pix_begin"]:b["pix_begin"] + b["n_pixels"]]
            want[int(r.info["blob_begin"]) + k] = oracle.posture_auto(rs, px, bg, 0, 15, pp)
    assert sum(oi["status"] == 0 for oi, _, _ in want) >= 10
    for n in (1, total, 1):
        gi, go, gs, gt, gn = posture_auto(seg, n)
        for k in range(n):
            oi, oo, osg = want[k]
            assert gn[k] == oi["iterations"] and gt[k] == oi["threshold"], (n, k, gn[k], gt[k], oi)
            assert gi[k]["status"] == oi["status"] and gi[k]["n_outline"] == oi["n_outline"], (n, k, gi[k], oi)
            assert go[k, :oi["n_outline"]].tobytes() == oo[:oi["n_outline"]].tobytes(), (n, k)
            if oi["status"] == 0:
                assert gi[k]["head_index"] == oi["head_index"] and gi[k]["n_segments"] == oi["n_segments"], (n, k, gi[k], oi)
                assert gs[k, :oi["n_segments"]].tobytes() == osg[:oi["n_segments"]].tobytes(), (n, k)


# ---- one buffer, two users: u64 timestamps per frame (pack.hip), a float per blob (midline.hip) ---------------------------------------------
def pack(seg, res):
    n = len(res)
    ts = np.arange(n, dtype=np.uint64) * 33333 + 0x0102030405060708
    want = [oracle.pv_serialize_v6(r.blobs, r.runs, r.pixels, int(t)) for r, t in zip(res, ts)]
    total = sum(len(w) for w in want)
    out = torch.zeros(total + 64, dtype=torch.uint8, device="cuda"); off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    seg.pack_frames_v6_device(out.data_ptr(), out.numel(), off.data_ptr(), ts)
    seg.synchronize()
    o = off.cpu().numpy(); got = out.cpu().numpy()
    assert int(o[n]) == total and np.array_equal(np.diff(o), [len(w) for w in want])
    for f in range(n):
        assert got[o[f]:o[f + 1]].tobytes() == want[f].tobytes(), f


def crops_posture(seg, res, fr, bg):
    total = sum(len(r.blobs) for r in res)
    outline = torch.zeros((total, MP, 2), dtype=torch.float32, device="cuda"); segs = torch.zeros((total, MP // 2 + 1, 4), dtype=torch.float32, device="cuda")
    info = torch.zeros((total, 8), dtype=torch.int32, device="cuda"); mid = torch.zeros((total, 25, 4), dtype=torch.float32, device="cuda")
    d_minfo = torch.zeros((total, 8), dtype=torch.int32, device="cuda")
    seg.posture_device(total, outline.data_ptr(), segs.data_ptr(), info.data_ptr(), max_points=MP)
    seg.midline_device(total, MP, info.data_ptr(), segs.data_ptr(), mid.data_ptr(), d_minfo.data_ptr())
    seg.synchronize()
    mi = d_minfo.cpu().numpy().view(capi.MIDLINE_INFO_DTYPE).reshape(-1)
    assert (mi["status"] == 0).sum() >= 2
    lengths = np.where(mi["status"] == 0, mi["len"] * 1.25 + 2.0 + np.arange(total), 30.0).astype(F)      # the caller's: none is the blob's own len()
    d = torch.full((total + 1, 32, 48, 1), 77, dtype=torch.uint8, device="cuda")
    seg.crops_posture_device(d.data_ptr(), total, d_minfo.data_ptr(), midline_lengths=lengths, out_w=48, out_h=32)
    seg.synchronize()
    got = d.cpu().numpy()
    assert (got[total] == 77).all()
    shown = 0
    for f, r in enumerate(res):
        for k, b in enumerate(r.blobs):
            bi = int(r.info["blob_begin"]) + k
            if mi[bi]["status"] != 0:
                assert not got[bi].any()
                continue
            tr = oracle.midline_transform(mi[bi]["angle"], mi[bi]["offx"], mi[bi]["offy"], False)
            want = oracle.crop_normalized(fr[f], bg, b, r.runs, out_w=48, out_h=32, difference=0, invert=False, nearest=False, tr6=tr,
                                          midline_length=float(lengths[bi]), legacy=False, scale=1.0)[0]
            assert got[bi, :, :, 0].tobytes() == want.tobytes(), bi
            shown += bool(want.any())
    assert shown >= 2


@pytest.mark.parametrize("order", ["pack_first", "crops_first"])
def test_timestamps_and_midline_lengths_share_a_buffer(seg, order):
    fr, bg = scene64([2, 1], 19)
    ctx = seg if order == "pack_first" else make_ctx()
    try:
        res = segment(ctx, fr, bg)
        assert sum(len(r.blobs) for r in res) == 3
        steps = [lambda: pack(ctx, res), lambda: crops_posture(ctx, res, fr, bg)]
        for step in (steps if order == "pack_first" else steps[::-1]):
            step()
    finally:
        if ctx is not seg:
            ctx.close()


# ---- the two table sets, fetched in turn ------------------------------------------------------------------------------------------------------
def test_fetch_and_fetch_rethreshold_alternate_over_two_batches():
    ctx = make_ctx(max_batch=20)
    thr, method, ranges = 60, 0, [(5, 400)]
    try:
        for counts, seed in (([3], 23), ([3, 4, 1, 2] * 5, 29)):            # 1 frame: the exporting kernel; 20 frames: the DMA path
            fr, bg = scene64(counts, seed)
            p = oracle.make_params(W, H)
            det_want = [oracle.segment(f, bg, p) for f in fr]
            sub_want = [oracle.rethreshold_frame(f, bg, p, method, thr, ranges) for f in fr]
            assert sum(len(ob) for ob, _, _ in sub_want) >= len(fr)
            det = segment(ctx, fr, bg)
            ctx.rethreshold(thr, method, ranges)
            for _ in range(2):
                sub = ctx.fetch(rethreshold=True)
                assert len(sub) == len(fr)
                for f, (r, (ob, orr, opx)) in enumerate(zip(sub, sub_want)):
                    assert r.runs.tobytes() == orr.tobytes() and r.pixels.tobytes() == opx.tobytes(), f
                    want = ob.copy()
                    want["parent"] = want["parent"] + det[f].info["blob_begin"]          # device parents are pooled indices
                    for name in ob.dtype.names:
                        assert r.blobs[name].tobytes() == want[name].tobytes(), (f, name)
                same_tables(ctx.fetch(), det_want)
    finally:
        ctx.close()


# ---- the network's per-batch buffers ----------------------------------------------------------------------------------------------------------
def test_identify_3_40_3_crops_equal_each_crop_alone(seg):
    classes = 8
    blob = weights.pack_blob(weights.synthetic_state(classes, 11), classes)
    crops = weights.synthetic_crops(40, 5)
    d_crops = torch.from_numpy(crops).cuda()
    fresh = make_ctx()
    try:
        fresh.load_weights(blob)
        alone = torch.zeros((40, classes), dtype=torch.float32, device="cuda")
        one = d_crops.numel() // 40
        for k in range(40):
            fresh.identify_device(d_crops.data_ptr() + k * one, 1, alone.data_ptr() + k * classes * 4)
        fresh.synchronize()
        alone = alone.cpu().numpy()
    finally:
        fresh.close()
    assert np.isfinite(alone).all() and np.abs(alone.sum(1) - 1).max() < 1e-5 and len({r.tobytes() for r in alone}) >= 2
    seg.load_weights(blob)
    for n in (3, 40, 3):
        probs = torch.full((n + 1, classes), -7.0, dtype=torch.float32, device="cuda")
        seg.identify_device(d_crops.data_ptr(), n, probs.data_ptr())
        seg.synchronize()
        got = probs.cpu().numpy()
        assert got[:n].tobytes() == alone[:n].tobytes(), n
        assert (got[n] == -7.0).all()
