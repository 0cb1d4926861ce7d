"""Paths of trex_amd/csrc/prefilter.hip that the hand-worked 64 x 48 scenes of test_prefilter_gpu.py do not reach, byte-equal to
tests/prefilter_ref.py: frame rows whose 16-byte alignment differs from the background's (k_pre_count2's byte-wise fallback), a frame with
more than 256 detect blobs, sub-blobs and sequence slots (the chunked scans and the rank cursor of k_pre_decide), and force_set_recount."""
import numpy as np
import pytest
import prefilter_cases as pc
import prefilter_ref as ref
import test_prefilter_gpu as base

pytestmark = pytest.mark.gpu


def _paint(W, H, rects):
    f = np.full((H, W), pc.BG, np.uint8)
    for x0, y0, x1, y1, v in rects:
        f[y0:y1 + 1, x0:x1 + 1] = v
    return f


def test_rows_aligned_differently_from_the_background():
    # 72 x 47 = 3384 bytes per frame = 8 mod 16: every row of frame 1 sits 8 bytes off the background's row, so lines of 32 pixels and more
    # take the byte-wise loop there and the 16-byte loop in frame 0; the counts must be the same
    W, H = 72, 47
    rects = [(3, 5, 60, 6, 160), (5, 5, 40, 5, 100), (9, 20, 71, 21, 160), (30, 21, 71, 21, 100), (2, 30, 34, 30, 100)]
    f = _paint(W, H, rects)
    frames, bg = np.stack([f, f]), np.full((H, W), pc.BG, np.uint8)
    st = ref.Settings(track_threshold=30, track_threshold_2=60, threshold_ratio_range=(0.0, 2.0))
    det, sub, got, want = base.check(frames, st, bg=bg, second_count=True)
    sec = got[0].second_count
    assert np.array_equal(sec, want[4])
    per_frame = [sorted(sec[fi * base.MAX_BLOBS:fi * base.MAX_BLOBS + len(sub[fi].blobs)].tolist()) for fi in range(2)]
    assert per_frame[0] == per_frame[1] == [33, 36, 42]
    assert max(int(r["x1"]) - int(r["x0"]) + 1 for r in sub[1].runs) >= 58


def many_blobs_frame(W=128, H=96):
    """300 small blobs on a grid of pitch 5 (2 x 2 = 4, 3 x 2 = 6 and 3 x 3 = 9 pixels, every eleventh one weak), and one tall blob at the
    right edge whose two strong ends are joined by a weak line: its two sub-blobs lie in different chunks of 256 table slots."""
    rects, k = [], 0
    for gy in range(H // 5):
        for gx in range(23):
            if k == 300:
                break
            w, h = ((2, 2), (3, 2), (3, 3))[k % 3]
            rects.append((1 + 5 * gx, 1 + 5 * gy, 1 + 5 * gx + w - 1, 1 + 5 * gy + h - 1, 180 if k % 11 == 0 else 100))
            k += 1
    assert k == 300
    rects += [(121, 6, 121, 90, 180), (120, 2, 122, 5, 100), (120, 91, 122, 93, 100)]       # 12 and 9 strong pixels
    return _paint(W, H, rects)


def test_a_frame_with_more_than_256_blobs():
    f = many_blobs_frame()
    frames, bg = np.stack([f, pc.paint(pc.SIZES).repeat(2, axis=0).repeat(2, axis=1)]), np.full(f.shape, pc.BG, np.uint8)
    st = ref.Settings(track_threshold=30, track_threshold_2=60, threshold_ratio_range=(0.5, 2.0), track_size_filter=[(5, 8), (12, 13)])
    det, sub, got, want = base.check(frames, st, bg=bg, max_blobs=512, calls=2, second_count=True)
    assert len(det[0].blobs) == 301 and len(sub[0].blobs) > 256
    tall = pc.blob_at(det[0], 121, 50)
    kids = np.nonzero(sub[0].blobs["parent"] == int(det[0].info["blob_begin"]) + tall)[0]
    assert len(kids) == 2 and kids[0] < 256 <= kids[1]
    c = want[2][0]
    assert c[0] > 80 and c[1] > 80 and c[2] > 80 and c[3] == 0 and c[:3].sum() > 256        # all three classes, more entries than one chunk
    assert np.array_equal(got[0].second_count, want[4])
    for name in ("decision", "order", "counts", "presumed_nr", "second_count"):
        assert getattr(got[0], name).tobytes() == getattr(got[1], name).tobytes(), name


def test_force_set_recount_far_above_the_largest_range():
    # 150 weak pixels: nothing survives track_threshold 30, so the counted recount would be 0 (OutsideRange below 0.1); at more than 100
    # times the largest range's end the reference sets the recount to every pixel without counting (Tracker.cpp:768-771) -> big
    scene = [(4, 4, 18, 13, 180)] + [(30, 30, 34, 34, 180)]                                  # 150 px > 1.0 * 100, and 25 px that is counted
    st = ref.Settings(track_threshold=30, track_size_filter=[(0.1, 1.0)])
    det, sub, got, want = base.check(base._batch(scene, pc.SIZES), st)
    cap, big, small = got[0].cap, pc.blob_at(det[0], 4, 4), pc.blob_at(det[0], 30, 30)
    assert want[0][cap + big] == ref.BIG and want[0][cap + small] == ref.FILTERED + ref.OUTSIDE_RANGE
    assert want[3][int(det[0].info["blob_begin"]) + big] == 2
