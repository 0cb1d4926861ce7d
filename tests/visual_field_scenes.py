"""Seeded synthetic scenes for the visual-field tests: outlines built directly as the d_outline / d_posture_info arrays of the posture call
(no segmentation), entries, observers, and the expected result from tests/visual_field_ref.py, computed once per scene and shared.

Every scene is checked against the restatement's fragility report when it is built: a scene with ONE fragile record (a projected value
within 1e-9 of an integer or of a field-of-view end, an angle within 1e-9 of +-pi before a correct_angle, two end angles within 1e-9 of
each other while the points differ) is refused -- the cap on excluded cases is zero, nothing is masked out of a comparison.  A seed that
trips the rule is moved here, on the CPU (tests/test_visual_field_cpp.py builds every scene without a GPU)."""
import functools
import math
import numpy as np
import visual_field_ref as R

MAXP = 96                                   # row length of the outline array (the posture call's max_points)
MAX_TESS = 512
INFO_DTYPE = np.dtype([("status", "<i4"), ("n_outline", "<i4"), ("n_segments", "<i4"), ("tail_index", "<i4"), ("head_index", "<i4"),
                       ("n_traced", "<i4"), ("reserved", "<i4", (2,))])          # trexhip_posture_info
CHUNK_RECORDS, LDS_RECORDS = 512, 1024      # what capi exports as VF_CHUNK_RECORDS / VF_LDS_RECORDS (the GPU test asserts they agree)


class Scene:
    def __init__(self, max_d=640.0 ** 2 + 480.0 ** 2, max_tess=MAX_TESS):
        self.rows, self.info_rows, self.entries, self.frame_entries, self.observers = [], [], [], [0], []
        self.max_d, self.max_tess, self.max_distance = max_d, max_tess, 5.0

    def row(self, pts, tail, head=None):
        pts = np.asarray(pts, np.float32).reshape(-1, 2)
        assert len(pts) <= MAXP
        r = np.zeros((MAXP, 2), np.float32)
        r[:len(pts)] = pts
        self.rows.append(r)
        self.info_rows.append((0, len(pts), 0, tail, (tail + len(pts) // 2) % max(len(pts), 1) if head is None else head, 0, (0, 0)))
        return len(self.rows) - 1

    def entry(self, ident, row, pos, flags=0):
        self.entries.append((ident, row, pos[0], pos[1], flags, 0))
        return len(self.entries) - 1

    def end_frame(self):
        self.frame_entries.append(len(self.entries))

    def observe(self, frame, entry, eyes, angles):
        self.observers.append((frame, entry, (eyes[0][0], eyes[1][0]), (eyes[0][1], eyes[1][1]), tuple(angles)))

    def arrays(self):
        return dict(outline=np.asarray(self.rows, np.float32).reshape(-1, MAXP, 2), info=np.array(self.info_rows, INFO_DTYPE),
                    frame_entries=np.array(self.frame_entries, np.int32), entries=np.array(self.entries, R.ENTRY_DTYPE),
                    observers=np.array(self.observers, R.OBSERVER_DTYPE), max_d=self.max_d, max_tess=self.max_tess, max_distance=self.max_distance)


def reference(a, report=None, max_tess=None):
    return R.cast(a["outline"], a["info"]["n_outline"], a["info"]["tail_index"], a["info"]["head_index"], a["frame_entries"], a["entries"],
                  a["observers"], a["max_d"], a["max_distance"], a["max_tess"] if max_tess is None else max_tess, report)


def ellipse(rng, n, a, b):
    """n points of an ellipse with semi-axes a, b at a random rotation, relative to its bounds' corner (all coordinates >= 0)"""
    t = np.sort(rng.uniform(0, 2 * math.pi, n))
    rot = rng.uniform(0, 2 * math.pi)
    x, y = a * np.cos(t), b * np.sin(t)
    p = np.stack([x * math.cos(rot) - y * math.sin(rot), x * math.sin(rot) + y * math.cos(rot)], 1)
    return (p - p.min(0)).astype(np.float32)


def wrap(a):
    return R.correct_angle(a)


def eyes_of(rng, pts, pos):
    """two eyes 2 px in front of the outline along a random heading, 1 to 4 px apart, looking 60 degrees to either side of the heading: each
    sees part of its own body behind it, as generate_eyes places them"""
    p = np.asarray(pts, np.float64)
    c = p.mean(0)
    h = rng.uniform(-math.pi, math.pi)
    front = c + np.array([math.cos(h), math.sin(h)]) * (np.sqrt(((p - c) ** 2).sum(1)).max() + 2.0) + np.asarray(pos, np.float64)
    off = np.array([-math.sin(h), math.cos(h)]) * rng.uniform(0.5, 2.0)
    return [tuple(front + off), tuple(front - off)], [wrap(h + math.radians(60)), wrap(h - math.radians(60))]


def ring(side_points, step):
    """an axis-aligned square outline with side_points points per side, `step` px apart: step 20 gives three inserts per edge"""
    s = side_points * step
    pts = [(i * step, 0) for i in range(side_points)] + [(s, i * step) for i in range(side_points)]
    pts += [(s - i * step, s) for i in range(side_points)] + [(0, s - i * step) for i in range(side_points)]
    return np.array(pts, np.float32)


BEHIND = [(-10.0, 1.0), (-10.0, -1.0), (-12.0, 0.5)]      # seen from an eye at its pos looking along +x: beyond +-130 degrees


def random_frames(seed, counts, observers_per_frame, specials=True):
    rng = np.random.default_rng(seed)
    sc = Scene()
    for f, cnt in enumerate(counts):
        first = len(sc.entries)
        made = []
        for k in range(cnt):
            n = int(rng.integers(8, 91))
            pts = ellipse(rng, n, rng.uniform(4, 40), rng.uniform(3, 15))
            pos = (float(np.float32(rng.uniform(20, 560))), float(np.float32(rng.uniform(20, 400))))
            tail, flags, row_pts = int(rng.integers(0, n)), 0, pts
            if specials and cnt >= 5:
                if k == 1:
                    row_pts = pts.copy(); row_pts[3] = row_pts[2]; row_pts[n - 1] = row_pts[0]      # duplicate outline points (pt0 == pt1)
                if k == 3:
                    flags = 1                                                                   # the midline was turned round: head_index is the tail
            row = sc.row(row_pts, tail)
            if specials and cnt >= 5 and k == 2:
                sc.info_rows[row] = sc.info_rows[row][:3] + (-1,) + sc.info_rows[row][4:]           # no tail index: skipped, in the middle of the list
            e = sc.entry(100 + 10 * f + k, -1 if (specials and cnt >= 5 and k == cnt - 2) else row, pos, flags)
            made.append((e, row_pts, pos))
        sc.end_frame()
        usable = [m for i, m in enumerate(made) if not (specials and cnt >= 5 and i in (2, cnt - 2))]
        for e, pts, pos in usable[:observers_per_frame[f]]:
            eyes, angles = eyes_of(rng, pts, pos)
            sc.observe(f, e, eyes, angles)
    return sc


def build(name):
    if name == "self":                       # 1 frame, 1 entry: the observer alone
        return random_frames(11, [1], [1], specials=False)
    if name == "occlude3":                   # one individual behind another as seen from the observer, a third elsewhere
        rng = np.random.default_rng(5)
        sc = Scene()
        o = ellipse(rng, 30, 20, 6)
        rows = [sc.row(o, 4), sc.row(ellipse(rng, 24, 12, 8), 2), sc.row(ellipse(rng, 40, 30, 14), 7)]
        e0 = sc.entry(1, rows[0], (100.0, 200.0))
        sc.entry(2, rows[2], (300.0, 185.0))             # far and large
        sc.entry(3, rows[1], (200.0, 195.0))             # near and small, in front of it, later in the list
        sc.end_frame()
        sc.observe(0, e0, [(150.3, 206.1), (150.2, 203.7)], [0.4, -0.35])     # in front of its own outline (x <= 140), looking along +x
        return sc
    if name == "two_frames":                 # 5 and 12 entries, a subset observes; skipped entries, flag bit 0, duplicate points
        return random_frames(23, [5, 12], [2, 4])
    if name in ("lds_exact", "lds_exceed"):
        # rings of 64 points, 20 px apart: 256 tessellated points = 512 records = exactly one compute step each, all inside the field of view
        # of an observer whose own outline lies behind its eyes.  Two rings: exactly LDS_RECORDS records wait in LDS; three: a flush
        # in the middle of the frame, and its third ring has more records than one step takes
        sc = Scene(max_d=4000.0 ** 2, max_tess=MAX_TESS)
        own = sc.entry(1, sc.row(BEHIND, 1), (0.0, 0.0))
        r = sc.row(ring(16, 20), 5)
        sc.entry(2, r, (500.0, -157.25))
        sc.entry(3, r, (900.0, -161.5))
        if name == "lds_exceed":
            sc.entry(4, sc.row(ring(16, 25), 9), (1400.0, -190.125))                         # 25 px apart: 320 tessellated points, two steps
        sc.end_frame()
        sc.observe(0, own, [(0.013, 0.021), (0.013, 0.021)], [0.05, 0.05])
        return sc
    if name == "spans":
        # (a) a two-point target 3 px from the eye whose ends sit at +-129.8 degrees (4.6 px apart: nothing is inserted): the line passes
        #     behind the eye, the record spans all 512 bins
        # (b) a small target around -97.75 degrees: its records cross bins 63 / 64, the boundary between the first two waves
        sc = Scene(max_d=1000.0 ** 2)
        own = sc.entry(1, sc.row(BEHIND, 0), (0.0, 0.0))
        a = math.radians(129.8)
        sc.entry(2, sc.row([(3 * math.cos(a), 3 * math.sin(a)), (3 * math.cos(a), -3 * math.sin(a))], 0), (0.0, 0.0))
        b = math.radians(-97.75)
        sc.entry(3, sc.row(ellipse(np.random.default_rng(2), 12, 6, 4), 3), (100 * math.cos(b) - 5, 100 * math.sin(b) - 4))
        sc.end_frame()
        sc.observe(0, own, [(0.0011, 0.0017), (0.0011, 0.0017)], [0.0, 0.0])
        return sc
    if name == "capacity":
        # frame 0 holds a ring of 256 tessellated points and is cast with max_tess_points 255; frame 1 is an ordinary frame
        sc = random_frames(31, [3, 4], [2, 2], specials=False)
        r = sc.row(ring(16, 20), 5)
        old = sc.entries[1]
        sc.entries[1] = (old[0], r) + tuple(old[2:])
        sc.max_tess = 255
        return sc
    raise KeyError(name)


NAMES = ("self", "occlude3", "two_frames", "lds_exact", "lds_exceed", "spans", "capacity")


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (arrays, expected, report); the scene is refused if it has a fragile record or misses what it was built to exercise"""
    a = build(name).arrays()
    rep = {}
    want = reference(a, rep)
    assert rep["fragile"] == [], f"scene {name}: fragile records {rep['fragile'][:3]} -- move the seed"
    kept = rep["kept"]
    if name == "occlude3":
        assert ((want["ids"][0, :, 0] == 3) & (want["ids"][0, :, 1] == 2)).any(), "nothing is occluded"
    if name == "two_frames":
        assert (want["status"] == 0).all() and (want["ids"][:, :, 1] >= 0).any()
    if name == "lds_exact":
        assert kept[(0, 0)] == LDS_RECORDS and kept[(0, 1)] == LDS_RECORDS, kept
    if name == "lds_exceed":
        assert kept[(0, 0)] > LDS_RECORDS + CHUNK_RECORDS, kept
    if name == "spans":
        assert (0, 511) in rep["spans"] and any(s <= 63 and e >= 64 and e - s < 64 for s, e in rep["spans"]), sorted(rep["spans"])[:8]
    if name == "capacity":
        f0 = a["observers"]["frame"] == 0
        assert (want["status"][f0] == 2).all() and (want["status"][~f0] == 0).all()
        assert R.tesselate(ring(16, 20), 5.0, 256) is not None and R.tesselate(ring(16, 20), 5.0, 255) is None
    for v in want.values():
        v.setflags(write=False)
    return a, want, rep
