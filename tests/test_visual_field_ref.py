"""Hand-worked cases of tests/visual_field_ref.py, the line-by-line restatement of track::VisualField (VisualField.cpp) that the device call and
the host twin are held to.  Every expectation below is worked out on paper from the reference's lines, not from running the restatement.

Geometry used throughout: an eye at the origin looking along +x (angle 0) maps the direction t (degrees) to the value (t + 130) / 260 * 512,
so straight ahead is exactly 256.  A line between the values a <= b touches the bins uint(max(0, a - 1)) .. ceil(min(511, b + 1)).
  atan(10 / 100) = 5.7106 deg -> 244.754 / 267.246        atan(10 / 110) = 5.1944 deg -> 245.771 / 266.229
  atan(10 / 200) = 2.8624 deg -> 250.363 / 261.637        atan(10 / 50) = 11.3099 deg -> 233.728 / 278.272
The observer's own outline is a small triangle behind the eye (directions beyond +-130 degrees) unless a case says otherwise, so it writes
nothing; max_distance is 1000 in the casting cases so that tessellation inserts nothing and the points are the ones written here."""
import math
import numpy as np
import visual_field_ref as R

MAXP = 8
BEHIND = [(-10, 1), (-10, -1), (-12, 0)]
SQUARE = [(0, -10), (10, -10), (10, 10), (0, 10)]            # with pos (100, 0): P0 (100,-10) P1 (110,-10) P2 (110,10) P3 (100,10)
INV = R.INVALID


def scene(individuals, observer=0, eye_angle=0.0, eye=(0.0, 0.0)):
    """individuals: list of (id, points, tail_index, pos); one frame, one observer with both eyes alike"""
    n = len(individuals)
    outline = np.zeros((n, MAXP, 2), np.float32)
    n_outline, tail, head = np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    entries = np.zeros(n, R.ENTRY_DTYPE)
    for k, (ident, pts, t, pos) in enumerate(individuals):
        outline[k, :len(pts)] = pts
        n_outline[k], tail[k] = len(pts), t
        entries[k] = (ident, k, pos[0], pos[1], 0, 0)
    obs = np.zeros(1, R.OBSERVER_DTYPE)
    obs[0] = (0, observer, (eye[0], eye[0]), (eye[1], eye[1]), (eye_angle, eye_angle))
    return dict(outline=outline, n_outline=n_outline, tail_index=tail, head_index=head, frame_entries=np.array([0, n], np.int32), entries=entries,
                observers=obs)


def cast(sc, max_d, max_distance=1000.0, **kw):
    out = R.cast(max_d=max_d, max_distance=max_distance, **sc, **kw)
    for k in ("depth", "ids", "points", "fov", "head_distance"):
        assert out[k][0, 0].tobytes() == out[k][0, 1].tobytes(), "both eyes are alike in these cases"
    return {k: (v[0, 0] if k != "status" else v) for k, v in out.items()}


def expect(out, layer, bins, depth, ident, point, fov, hd):
    """the bins hold exactly this, every other bin of the layer the values of eye::eye()"""
    lo, hi = bins
    want_depth = np.full(512, INV); want_depth[lo:hi + 1] = depth
    want_ids = np.full(512, -1, np.int32); want_ids[lo:hi + 1] = ident
    want_pts = np.zeros((512, 2), np.float32); want_pts[lo:hi + 1] = point
    want_fov = np.zeros(512, np.uint8); want_fov[lo:hi + 1] = fov
    want_hd = np.full(512, -1.0); want_hd[lo:hi + 1] = hd
    assert np.array_equal(out["depth"][layer], want_depth), np.flatnonzero(out["depth"][layer] != want_depth)
    assert np.array_equal(out["ids"][layer], want_ids)
    assert np.array_equal(out["points"][layer], want_pts)
    assert np.array_equal(out["fov"][layer], want_fov), out["fov"][layer][lo:hi + 1]
    assert np.array_equal(out["head_distance"][layer], want_hd)


def untouched(out, layer):
    expect(out, layer, (0, -1), 0, 0, (0, 0), 0, 0)


def test_initial_values_are_those_of_eye():
    e = R.Eye()
    assert e.depth == [float(np.finfo(np.float32).max)] * 1024 and e.ids == [-1] * 1024 and e.fov == [0] * 1024 and e.hd == [-1.0] * 1024


def test_square_straight_ahead():
    # the first record (P3, P0) spans -5.71 .. 5.71 degrees: 243.754 -> 243, ceil(268.246) = 269, d = 100^2 + 10^2 from rp = pt0 = P3; no later
    # record is nearer (P1, P2 are at 110^2 + 10^2) and none reaches further, one id never enters layer 2.
    # fov = uchar((1 - 10100 / 40400)^2 * 255) = uchar(0.5625 * 255) = 143; hd at i = 0 with T_obs = 0: (1 - 0 / (right + 1)) * 255 = 255
    out = cast(scene([(1, BEHIND, 0, (0, 0)), (7, SQUARE, 0, (100, 0))]), max_d=40400.0)
    assert out["status"][0] == 0
    expect(out, 0, (243, 269), 10100.0, 7, (100, 10), 143, 255.0)
    untouched(out, 1)


def two_targets(order):
    near, far = (7, SQUARE, 0, (100, 0)), (8, SQUARE, 0, (200, 0))
    return cast(scene([(1, BEHIND, 0, (0, 0))] + ([near, far] if order == "near-first" else [far, near])), max_d=404000.0)


def check_two_targets(out):
    # layer 1: the near square as above, fov = uchar(0.975^2 * 255) = uchar(242.41) = 242
    # layer 2: the far square, first record +-2.8624 degrees: 249.363 -> 249, ceil(262.637) = 263, d = 200^2 + 10^2, rp = (200, 10),
    #          fov = uchar((1 - 40100 / 404000)^2 * 255) = uchar(206.89) = 206
    expect(out, 0, (243, 269), 10100.0, 7, (100, 10), 242, 255.0)
    expect(out, 1, (249, 263), 40100.0, 8, (200, 10), 206, 255.0)


def test_two_targets_on_one_ray_nearer_first():
    # the far one arrives second: depth[i] > d fails, it is another id than layer 1's and nearer than layer 2's FLT_MAX -> layer 2 (:137-145)
    check_two_targets(two_targets("near-first"))


def test_two_targets_on_one_ray_farther_first():
    # the far one holds layer 1 until the near one arrives and pushes it down (:114-122); the near square's later records find their own id in
    # layer 1 and leave layer 2 alone.  Same picture by another path
    check_two_targets(two_targets("far-first"))


def test_own_outline_in_front_invalidates_layer_2():
    # entries: far (8), near (7), then the observer itself (1) as a square at x = 50..60: first record +-11.31 degrees -> 232 .. 280, d = 2600.
    # Where the near square held layer 1 (243 .. 269) it is pushed to layer 2 -- over the far one, which is farther -- and then the self hit
    # sets that layer-2 depth back to FLT_MAX while ids, points, fov and head distance stay (:131-135).  Elsewhere layer 1 was empty
    # (id -1, depth FLT_MAX > FLT_MAX fails): nothing moves down.
    sc = scene([(8, SQUARE, 0, (200, 0)), (7, SQUARE, 0, (100, 0)), (1, SQUARE, 0, (50, 0))], observer=2)
    out = cast(sc, max_d=404000.0)
    fov_self = int((1 - 2600 / 404000) ** 2 * 255)                 # 251.7 -> 251
    assert fov_self == 251
    expect(out, 0, (232, 280), 2600.0, 1, (50, 10), 251, 255.0)
    expect(out, 1, (243, 269), INV, 7, (100, 10), 242, 255.0)


def test_target_behind_the_eye_writes_nothing():
    out = cast(scene([(1, BEHIND, 0, (0, 0)), (7, SQUARE, 0, (-120, 0))]), max_d=40400.0)
    assert out["status"][0] == 0
    untouched(out, 0)
    untouched(out, 1)


def test_target_straddling_the_seam():
    # the eye looks along -x (angle pi); the square's near corners (-100, +-10) have atan2 = +-174.29 degrees, on both sides of the seam.
    # 174.29 - 180 = -5.71; -174.29 - 180 = -354.29 -> correct_angle -> 5.71: the picture of the first case, mirrored.
    # P3 = (-100, 10) is pt0 of the first record
    mirrored = [(0, -10), (-10, -10), (-10, 10), (0, 10)]
    sc = scene([(1, [(10, 1), (10, -1), (12, 0)], 0, (0, 0)), (7, mirrored, 0, (-100, 0))], eye_angle=math.pi)
    out = cast(sc, max_d=40400.0)
    expect(out, 0, (243, 269), 10100.0, 7, (-100, 10), 143, 255.0)
    untouched(out, 1)


def test_target_crossing_a_field_of_view_edge():
    # two points: Pa = (-50, 87) at 119.886 degrees -> 492.083, Pb = (-77, 64) at 140.27 degrees, outside -> -1.  n = 2: previous = Pb, ptp = Pa.
    # i = 0: (Pb, Pa): first = 492.083 (the smaller angle is Pa's), second = -1; first >= 0 -> rp = pt0 = Pb although Pb is the end outside;
    #        d = 77^2 + 64^2 = 10025; x0 = 491.083, x1 = -1 -> x0: bins 491 .. ceil(491.083) = 492
    #        (Pa, Pa): 492.083 twice, rp = Pa, d = 50^2 + 87^2 = 10069: bins 491 .. ceil(493.083) = 494; 491 and 492 are nearer already
    # i = 1: (Pa, Pb): rp = Pa, d = 10069 over 491 .. 492: not nearer.  (Pb, Pb): outside
    out = cast(scene([(1, BEHIND, 0, (0, 0)), (7, [(-50, 87), (-77, 64)], 0, (0, 0))]), max_d=1e12)
    want_d = np.full(512, INV); want_d[491:493] = 10025.0; want_d[493:495] = 10069.0
    want_p = np.zeros((512, 2), np.float32); want_p[491:493] = (-77, 64); want_p[493:495] = (-50, 87)
    assert np.array_equal(out["depth"][0], want_d) and np.array_equal(out["points"][0], want_p)
    assert np.array_equal(np.flatnonzero(out["ids"][0] == 7), np.arange(491, 495))
    assert np.array_equal(out["head_distance"][0][491:495], np.full(4, 255.0))
    assert np.array_equal(out["fov"][0][491:495], np.full(4, 254, np.uint8))       # (1 - 1e-8)^2 * 255 = 254.99999 -> 254
    untouched(out, 1)


def test_tessellation_of_a_square_with_12_px_sides():
    # L = 12 > 5: N = 12 / 5 + 0.5 = 2.9, i < 1.9: one insert per edge at previous + direction * 5; previous starts as the last point
    got = R.tesselate(np.array([(0, 0), (12, 0), (12, 12), (0, 12)], np.float32))
    assert got == [(0, 7), (0, 0), (5, 0), (12, 0), (12, 5), (12, 12), (7, 12), (0, 12)]
    # 16 px: N = 3.7, i < 2.7: two inserts; 7.5 px: N = 2.0, i < 1.0: none although L > 5; 5 px: L > 5 fails
    got = R.tesselate(np.array([(0, 0), (16, 0), (16, 7.5), (16, 12.5)], np.float32))
    assert got[-3:] == [(16, 0), (16, 7.5), (16, 12.5)]
    assert got[3:6] == [(0, 0), (5, 0), (10, 0)]                                           # the two inserts of the 16 px edge
    # the closing edge (16, 12.5) -> (0, 0): L = sqrtf(412.25) = 20.30..., N = 4.56, i < 3.56: three inserts, in float32
    assert len(got) == 9
    f = np.float32
    dx, dy = f(-16), f(-12.5)
    L = f(np.sqrt(f(dx * dx + dy * dy)))
    ux, uy = f(dx / L), f(dy / L)
    assert got[0] == (float(f(f(16) + f(f(ux * f(1)) * f(5)))), float(f(f(12.5) + f(f(uy * f(1)) * f(5)))))
    # the device's capacity: more than `limit` points is reported, never cut
    assert R.tesselate(np.array([(0, 0), (12, 0), (12, 12), (0, 12)], np.float32), limit=7) is None
    assert len(R.tesselate(np.array([(0, 0), (12, 0), (12, 12), (0, 12)], np.float32), limit=8)) == 8


NEAR_THEN_FAR = [(100, 0), (118, 21)]       # P0 straight ahead (256 exactly, d = 10000), P1 at 10.091 degrees (275.87, d = 14365)


def two_point_target(tail_target, observer_outline, tail_obs):
    # n = 2: previous = P1, ptp = P0.
    # i = 0: (P1, P0): first = 256 (P0's angle), rp = pt0 = P1, d = 14365: bins 255 .. ceil(276.87) = 277
    #        (P0, P0): rp = P0, d = 10000: bins 255 .. 257                                   <- written at i = 0
    # i = 1: (P0, P1): rp = P0, d = 10000 over 255 .. 277: nearer on 258 .. 277             <- written at i = 1
    #        (P1, P1): d = 14365: nothing
    out = cast(scene([(1, observer_outline, tail_obs, (0, 0)), (7, NEAR_THEN_FAR, tail_target, (0, 0))]), max_d=1e12)
    expect_d = np.full(512, INV); expect_d[255:278] = 10000.0
    assert np.array_equal(out["depth"][0], expect_d)
    assert np.array_equal(out["points"][0][255:278], np.tile(np.float32([100, 0]), (23, 1)))
    return out["head_distance"][0]


def test_left_side_zero_is_replaced():
    # tail index 2 = n: right = 3, left = n - T = 0 -> replaced by n - right = -1 (:435), so for i > T_obs the divisor left + 1 is 0:
    # hd = (1 - 1 / 0) * 255 = -inf.  Without the replacement it would be (1 - 1 / 1) * 255 = 0
    hd = two_point_target(2, BEHIND, 0)
    assert np.array_equal(hd[255:258], np.full(3, 255.0))                            # i = 0: (1 - 0 / (right + 1)) * 255
    assert np.array_equal(hd[258:278], np.full(20, -math.inf))


def test_head_distance_uses_the_observers_tail_index():
    # target: T = 0, right = 1, left = 2.  Observer: tail index 5.  i = 0: (1 - |0 - 5| / (right + 1)) * 255 = -382.5 (0 > 5 fails: right);
    # i = 1: (1 - 4 / 2) * 255 = -255.  With the target's own tail index it would be 255 and (1 - 1 / 3) * 255 = 170
    behind8 = [(-10, 1), (-10, -1), (-11, -1), (-12, -1), (-13, 0), (-12, 1), (-11, 1), (-10.5, 1)]
    hd = two_point_target(0, behind8, 5)
    assert np.array_equal(hd[255:258], np.full(3, -382.5))
    assert np.array_equal(hd[258:278], np.full(20, -255.0))


def test_unused_entries_and_status():
    sc = scene([(1, BEHIND, 0, (0, 0)), (7, SQUARE, 0, (100, 0)), (8, SQUARE, -1, (60, 0)), (9, SQUARE, 0, (50, 0))])
    sc["entries"]["posture_row"][3] = -1                     # no outline; entry 2 has no tail index: both are skipped
    out = cast(sc, max_d=40400.0)
    expect(out, 0, (243, 269), 10100.0, 7, (100, 10), 143, 255.0)
    # flag bit 0: head_index stands for the tail; with head_index -1 the observer itself is unusable -> status 1, initial values
    sc["entries"]["flags"][0] = 1
    out = cast(sc, max_d=40400.0)
    assert out["status"][0] == 1
    untouched(out, 0)
    # capacity: the 20 px sides of the square and the 10 px sides need 4 + 3 + 1 + 3 + 1 = 12 points at max_distance 5 -> status 2 with 11, fine with 12
    sc["entries"]["flags"][0] = 0
    assert cast(sc, max_d=40400.0, max_distance=5.0, max_tess_points=11)["status"][0] == 2
    assert cast(sc, max_d=40400.0, max_distance=5.0, max_tess_points=12)["status"][0] == 0


def test_fragility_report_names_a_record_on_an_integer():
    # P0 of the two-point target sits at 256 exactly: the report must say so (the GPU scenes are chosen to have no such record)
    rep = {}
    R.cast(max_d=1e12, max_distance=1000.0, report=rep, **scene([(1, BEHIND, 0, (0, 0)), (7, NEAR_THEN_FAR, 0, (0, 0))]))
    assert any("integer" in r[5] for r in rep["fragile"])
    # BEHIND has a point on the negative x axis, atan2 = pi exactly: the seam rule names it
    assert any("seam" in r[5] and r[2] == 0 for r in rep["fragile"])
    rep = {}
    R.cast(max_d=40400.0, max_distance=1000.0, report=rep, **scene([(1, [(-10, 1), (-10, -1), (-12, 0.5)], 0, (0, 0)), (7, SQUARE, 0, (100, 0.25))]))
    assert rep["fragile"] == []
