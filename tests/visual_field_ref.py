"""track::VisualField's cast, restated line by line in plain Python / float64 (float32 where the reference's Vec2 is float32).

Written from the reference (Application/src/tracker/tracking/VisualField.cpp, VisualField.h), not from the kernel: it is what
trexhip_visual_field_device and HipVisualField::cast_host are held to, byte for byte.

  tesselate      VisualField::tesselate_outline      :339-359
  project        project_angles_1d + correct_angle   :67-94
  plot           VisualField::plot_projected_line    :96-150
  cast           the loop over active individuals and the add_line lambda  :427-496, :526-576

Readings of what the reference leaves to the un-vendored commons (UNPINNED; include/trexhip.h names the same ones):
  Vec2 arithmetic     pt - previous, length() = sqrtf(x * x + y * y), direction /= L, previous + direction * i * max_distance: every
                      operation a float32 operation rounded on its own, i and max_distance converted to float32 first
  atan2(Vec64)        atan2(v.y, v.x)
  long_t              int32_t
  RADIANS(130)        130 * (M_PI / 180) in double
"""
import math
import numpy as np

RESOLUTION = 512
LAYERS = 2
INVALID = float(np.finfo(np.float32).max)          # VisualField::invalid_value = FLT_MAX as a double
SYMMETRIC_FOV = 130.0 * (math.pi / 180.0)
FOV_START, FOV_END = -SYMMETRIC_FOV, SYMMETRIC_FOV
FOV_LEN = FOV_END - FOV_START
TWO_PI = 2.0 * math.pi
EPS = 1e-9
_MASK64 = (1 << 64) - 1

ENTRY_DTYPE = np.dtype([("id", "<i4"), ("posture_row", "<i4"), ("pos_x", "<f4"), ("pos_y", "<f4"), ("flags", "<i4"), ("reserved", "<i4")])
OBSERVER_DTYPE = np.dtype([("frame", "<i4"), ("entry", "<i4"), ("eye_x", "<f8", (2,)), ("eye_y", "<f8", (2,)), ("eye_angle", "<f8", (2,))])
assert ENTRY_DTYPE.itemsize == 24 and OBSERVER_DTYPE.itemsize == 56


def _div(a, b):
    """a / b as C does it for doubles (a zero divisor gives an infinity or NaN, no exception)"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def tesselate(outline, max_distance=5.0, limit=None):
    """tesselate_outline (:339-359) on float32 points [n][2]; returns the list of (x, y) doubles, or None as soon as it holds more than
    `limit` points (the device's capacity; the reference has none)."""
    f32 = np.float32
    pts = [(f32(p[0]), f32(p[1])) for p in outline]
    out = []
    if not pts:
        return out
    px, py = pts[-1]                                              # auto previous = outline.back()
    md = f32(max_distance)
    with np.errstate(all="ignore"):
        for x, y in pts:
            dx, dy = f32(x - px), f32(y - py)                     # direction = pt - previous
            L = f32(np.sqrt(f32(f32(dx * dx) + f32(dy * dy))))    # direction.length()
            if float(L) > max_distance:
                dx, dy = f32(dx / L), f32(dy / L)                 # direction /= L
                N = float(L) / max_distance + 0.5
                i = 1
                while i < N - 1:                                  # for (int i = 1; i < N - 1; ++i)
                    fi = f32(i)
                    out.append((float(f32(px + f32(f32(dx * fi) * md))), float(f32(py + f32(f32(dy * fi) * md)))))
                    i += 1
                    if limit is not None and len(out) > limit:
                        return None
            out.append((float(x), float(y)))
            if limit is not None and len(out) > limit:
                return None
            px, py = x, y
    return out


def correct_angle(a):
    while a > math.pi:
        a -= TWO_PI
    while a <= -math.pi:
        a += TWO_PI
    return a


def _near_pi(a):
    return abs(abs(a) - math.pi) <= EPS


def project(ref_angle, angle0, angle1, fragile=None, points_differ=True):
    """project_angles_1d (:74-94).  Returns (first, second) after the swap.  `fragile`, a list, receives the names of the rules of the
    fragility report this record trips: a 1-ulp change of an atan2 could change a decision there."""
    if fragile is not None and (_near_pi(angle0) or _near_pi(angle1)):
        fragile.append("seam")
    angle0 = correct_angle(angle0)
    angle1 = correct_angle(angle1)
    angle0 = angle0 - ref_angle
    angle1 = angle1 - ref_angle
    if fragile is not None and (_near_pi(angle0) or _near_pi(angle1)):
        fragile.append("seam")
    angle0 = correct_angle(angle0)
    angle1 = correct_angle(angle1)
    if fragile is not None and points_differ and abs(angle0 - angle1) <= EPS:
        fragile.append("equal-angles")
    if angle1 < angle0:
        angle0, angle1 = angle1, angle0
    out = []
    for a in (angle0, angle1):
        if fragile is not None and (abs(a - FOV_START) <= EPS or abs(a - FOV_END) <= EPS):
            fragile.append("fov-end")
        if FOV_START <= a <= FOV_END:
            v = (a - FOV_START) / FOV_LEN * float(RESOLUTION)
            if fragile is not None and abs(v - round(v)) <= EPS:
                fragile.append("integer")
            out.append(v)
        else:
            out.append(-1.0)
    return out[0], out[1]


class Eye:
    """eye::eye() (VisualField.h:37-43): the initial values"""

    def __init__(self):
        n = RESOLUTION * LAYERS
        self.depth = [INVALID] * n
        self.ids = [-1] * n
        self.points = [(np.float32(0), np.float32(0))] * n
        self.fov = [0] * n
        self.hd = [-1.0] * n


def _fov_of(d, max_d):
    v = 1.0 - min(1.0, max(0.0, _div(d, max_d)))
    return int(v * v * 255)                                      # uchar(SQR(...) * 255): truncated


def span(first, second):
    """the bins start .. end of plot_projected_line (:98-107) for a record that is not (-1, -1)"""
    x0, x1 = first, second
    x0 = x1 if x0 == -1.0 else max(0.0, x0 - 1.0)                 # :102, before :103
    x1 = x0 if x1 == -1.0 else min(float(RESOLUTION) - 1.0, x1 + 1.0)
    return int(max(0.0, x0)), int(min(float(RESOLUTION), math.ceil(x1)))


def plot(e, first, second, d, rp, ident, hd, fish_id, max_d, ties=None):
    """plot_projected_line (:96-150)"""
    R = RESOLUTION
    if first == second and first == -1:
        return
    start, end = span(first, second)
    point = (np.float32(rp[0]), np.float32(rp[1]))
    i = start
    while i <= end and i < R:
        if e.depth[i] > d:
            if e.ids[i] != fish_id and e.ids[i] != ident and e.depth[i + R] > e.depth[i]:
                e.depth[i + R] = e.depth[i]
                e.ids[i + R] = e.ids[i]
                e.points[i + R] = e.points[i]
                e.fov[i + R] = e.fov[i]
                e.hd[i + R] = e.hd[i]
            e.depth[i] = d
            e.ids[i] = ident
            e.points[i] = point
            e.fov[i] = _fov_of(d, max_d)
            e.hd[i] = hd
            if ident == fish_id:                                  # remove 2. stage after self occlusions
                if e.depth[i + R] != INVALID:
                    e.depth[i + R] = INVALID
        else:
            if ties is not None and e.depth[i] == d and e.ids[i] != ident:
                ties.append(i)
            if e.ids[i] != fish_id and ident != e.ids[i] and e.depth[i + R] > d:
                e.depth[i + R] = d
                e.ids[i + R] = ident
                e.points[i + R] = point
                e.fov[i + R] = _fov_of(d, max_d)
                e.hd[i + R] = hd
        i += 1


def _tail(entry, tail_index, head_index):
    row = int(entry["posture_row"])
    return int(head_index[row]) if int(entry["flags"]) & 1 else int(tail_index[row])


def entry_used(entry, n_outline, tail_index, head_index):
    """:552 -- an outline, a midline, and a tail index that is set"""
    row = int(entry["posture_row"])
    return row >= 0 and int(n_outline[row]) > 0 and _tail(entry, tail_index, head_index) != -1


def add_line(eyes, eye_pos, eye_angle, ident, pos, points, T_target, T_obs, fish_id, max_d, on_record=None):
    """the add_line lambda (:427-496) for one target; left / right come from the TARGET's tail index (:571-572), hd from the OBSERVER's (:460)"""
    n = len(points)
    if n == 0:
        return
    right = float(T_target + 1)
    left = float((n - T_target) & _MASK64)                       # size_t arithmetic, then Scalar64
    if left == 0:
        left = float(n) - right
    if right == 0:
        right = float(n) - left
    previous = points[n - 1]
    ptp = points[((n - 2) & _MASK64) % n]
    for i in range(n):
        pt1 = points[i]
        for pair, pt0 in enumerate((previous, ptp)):
            hd = 1 - _div(abs(float(i) - float(T_obs)), (left if i > T_obs else right) + 1)
            hd *= 255
            for j in range(2):
                ex, ey = eye_pos[j]
                rx, ry = pos[0] - ex, pos[1] - ey                 # e.rpos = pos - e.pos
                l0 = (pt0[0] + rx, pt0[1] + ry)
                l1 = (pt1[0] + rx, pt1[1] + ry)
                fragile = [] if on_record is not None else None
                first, second = project(eye_angle[j], math.atan2(l0[1], l0[0]), math.atan2(l1[1], l1[0]), fragile, pt0 != pt1)
                ties = [] if on_record is not None else None
                if first >= 0 or second >= 0:
                    rp = (pt0[0] + pos[0], pt0[1] + pos[1]) if first >= 0 else (pt1[0] + pos[0], pt1[1] + pos[1])
                    d = (rp[0] - ex) * (rp[0] - ex) + (rp[1] - ey) * (rp[1] - ey)
                    plot(eyes[j], first, second, d, rp, ident, hd, fish_id, max_d, ties)
                if on_record is not None:
                    on_record(j, i, pair, first, second, fragile, ties)
        ptp = previous
        previous = pt1


def cast(outline, n_outline, tail_index, head_index, frame_entries, entries, observers, max_d, max_distance=5.0, max_tess_points=None,
         report=None):
    """trexhip_visual_field_device on host arrays.  outline float32 [rows][max_points][2]; n_outline / tail_index / head_index per row;
    frame_entries [n_frames + 1]; entries ENTRY_DTYPE; observers OBSERVER_DTYPE.  Returns depth, ids, points, fov, head_distance
    ([n_observers][2][2][512]) and status.  `report`, a dict, receives "fragile" (records a 1-ulp change of an atan2 could change) and
    "ties" (exact depth ties between different ids: order-resolved, listed for information), "kept" and "spans" (what the scenes
    are chosen by)."""
    no = len(observers)
    out = {
        "depth": np.full((no, 2, LAYERS, RESOLUTION), INVALID, np.float64),
        "ids": np.full((no, 2, LAYERS, RESOLUTION), -1, np.int32),
        "points": np.zeros((no, 2, LAYERS, RESOLUTION, 2), np.float32),
        "fov": np.zeros((no, 2, LAYERS, RESOLUTION), np.uint8),
        "head_distance": np.full((no, 2, LAYERS, RESOLUTION), -1.0, np.float64),
        "status": np.zeros(no, np.int32),
    }
    if report is not None:
        report.setdefault("fragile", [])
        report.setdefault("ties", [])
        report.setdefault("kept", {})                    # records per (observer, eye) that reach plot_projected_line
        report.setdefault("spans", set())                # their (start, end)
    tess = {}

    def tess_of(k):
        if k not in tess:
            e = entries[k]
            tess[k] = tesselate(outline[int(e["posture_row"]), :int(n_outline[int(e["posture_row"])])], max_distance, max_tess_points)
        return tess[k]

    for o in range(no):
        ob = observers[o]
        f, own = int(ob["frame"]), int(ob["entry"])
        lo, hi = int(frame_entries[f]), int(frame_entries[f + 1])
        assert lo <= own < hi, "observer outside its frame"
        used = [k for k in range(lo, hi) if entry_used(entries[k], n_outline, tail_index, head_index)]
        if any(tess_of(k) is None for k in used):
            out["status"][o] = 2
            continue
        if own not in used:
            out["status"][o] = 1
            continue
        T_obs = _tail(entries[own], tail_index, head_index)
        fish_id = int(entries[own]["id"])
        eyes = [Eye(), Eye()]
        eye_pos = [(float(ob["eye_x"][j]), float(ob["eye_y"][j])) for j in range(2)]
        eye_angle = [float(ob["eye_angle"][j]) for j in range(2)]
        for k in used:
            e = entries[k]
            on_record = None
            if report is not None:
                def on_record(j, i, pair, first, second, fragile, ties, k=k):
                    if first >= 0 or second >= 0:
                        report["kept"][(o, j)] = report["kept"].get((o, j), 0) + 1
                        report["spans"].add(span(first, second))
                    if fragile:
                        report["fragile"].append((o, j, k, i, pair, tuple(fragile)))
                    if ties:
                        report["ties"].append((o, j, k, i, pair, tuple(ties)))
            add_line(eyes, eye_pos, eye_angle, int(e["id"]), (float(e["pos_x"]), float(e["pos_y"])), tess_of(k),
                     _tail(e, tail_index, head_index), T_obs, fish_id, float(max_d), on_record)
        for j in range(2):
            out["depth"][o, j] = np.asarray(eyes[j].depth, np.float64).reshape(LAYERS, RESOLUTION)
            out["ids"][o, j] = np.asarray(eyes[j].ids, np.int64).astype(np.int32).reshape(LAYERS, RESOLUTION)
            out["points"][o, j] = np.asarray(eyes[j].points, np.float32).reshape(LAYERS, RESOLUTION, 2)
            out["fov"][o, j] = np.asarray(eyes[j].fov, np.uint8).reshape(LAYERS, RESOLUTION)
            out["head_distance"][o, j] = np.asarray(eyes[j].hd, np.float64).reshape(LAYERS, RESOLUTION)
    return out
