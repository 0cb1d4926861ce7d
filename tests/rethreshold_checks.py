"""Byte-for-byte comparisons of the device's re-threshold tables (fetch(rethreshold=True)) with the oracle's, shared by
tests/test_rethreshold_gpu.py and tests/test_rethreshold_paths_gpu.py."""
import numpy as np
from oracle import oracle

OWN_FIELDS = ("run_begin", "pix_begin", "parent", "flags")           # what a sub-blob carries about its place in a table, not about itself


def rebased(sub, det):
    """a frame's sub-blob tables as bytes, `parent` counted from the frame's first detect blob: equal for equal frames in any slot of a batch"""
    b = sub.blobs.copy()
    b["parent"] -= det.info["blob_begin"]
    return b.tobytes(), sub.runs.tobytes(), sub.pixels.tobytes()


def assert_sub_equal(sub, det, want):
    """sub, det: one frame's FrameResult of pass 2 and of the detect pass; want: oracle.rethreshold_frame's (blobs, runs, pixels)"""
    ob, orr, opx = want
    assert sub.info["flags"] == 0 and det.info["flags"] == 0
    assert sub.info["n_raw_runs"] == len(orr)                           # every sub-run is kept (pass 2 classifies, it drops nothing)
    assert len(sub.blobs) == len(ob), (len(sub.blobs), len(ob))
    assert sub.runs.tobytes() == orr.tobytes() and sub.pixels.tobytes() == opx.tobytes()
    got = sub.blobs.copy()
    got["parent"] -= det.info["blob_begin"]                             # device parents are pooled indices
    for name in ob.dtype.names:
        assert np.array_equal(got[name], ob[name]), name
    assert got.tobytes() == ob.tobytes()


def size_class(n_pixels, ranges, cm_per_pixel=1.0):
    """Tracker.cpp:864-912 on a recount: 0 in a range, 1 below the smallest range (TREXHIP_BLOB_BELOW_RANGE), 2 otherwise (TREXHIP_BLOB_BIG)"""
    if not ranges:
        return 0
    v = float(np.float32(n_pixels) * np.float32(cm_per_pixel * cm_per_pixel))
    if any(a <= v < b for a, b in ranges):
        return 0
    return 1 if v < min(a for a, _ in ranges) else 2


def assert_per_blob_equal(det, sub, bg, thr, method, ranges=(), cm_per_pixel=1.0, connectivity=8):
    """det, sub: one frame's detect and pass-2 FrameResult after rethreshold_per_blob; thr: the frame's share of the thresholds.  Every detect blob's
    sub-blobs are oracle.threshold_blob's of its own lines and pixels: matched by bid, then lines, pixels and every field that describes the blob.
    cm_per_pixel, connectivity: the context's detect settings, which the pass takes over"""
    assert sub.info["flags"] == 0 and det.info["flags"] == 0
    seen = 0
    for k, b in enumerate(det.blobs):
        mine = sub.blobs[sub.blobs["parent"] == det.info["blob_begin"] + k]
        seen += len(mine)
        if thr[k] < 0:
            assert len(mine) == 0
            continue
        rs = det.runs[b["run_begin"]:b["run_begin"] + b["n_runs"]]
        px = det.pixels[b["pix_begin"]:b["pix_begin"] + b["n_pixels"]]
        ob, orr, opx = oracle.threshold_blob(rs, px, bg, method, int(thr[k]), connectivity)
        assert sorted(mine["n_pixels"].tolist()) == sorted(ob["n_pixels"].tolist())
        assert sorted(mine["bid"].tolist()) == sorted(ob["bid"].tolist())
        assert len(set(ob["bid"].tolist())) == len(ob), "two sub-blobs of one parent share a bid: the scene cannot match them"
        by_bid = {int(o["bid"]): o for o in ob}
        for m in mine:
            o = by_bid[int(m["bid"])]
            assert sub.runs[m["run_begin"]:m["run_begin"] + m["n_runs"]].tobytes() == orr[o["run_begin"]:o["run_begin"] + o["n_runs"]].tobytes()
            assert sub.pixels[m["pix_begin"]:m["pix_begin"] + m["n_pixels"]].tobytes() == opx[o["pix_begin"]:o["pix_begin"] + o["n_pixels"]].tobytes()
            for name in ob.dtype.names:
                if name not in OWN_FIELDS:
                    assert m[name] == o[name], (k, name)
            assert m["flags"] == size_class(int(m["n_pixels"]), ranges, cm_per_pixel), (k, int(m["n_pixels"]))
    assert seen == len(sub.blobs)                                       # no sub-blob without a parent of this frame
