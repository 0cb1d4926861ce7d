"""Plain-Python restatement of Tracker::prefilter's blob policy, line by line: tracking/Tracker.cpp:742-914, PrefilterBlobs.cpp:130-150 and
:328-385, core/SizeFilters.cpp.  Works on the per-frame tables trexhip_fetch / trexhip_fetch_rethreshold return (capi.FrameResult, or the
oracle's tables with frame-local parents).  Test infrastructure only: the product never imports it.

Float types as in the reference: Float2_t = float (np.float32 here, every product and sum rounded on its own), size ranges Range<double>.
What the reference takes from the un-vendored commons is restated as include/trexhip.h lists it under UNPINNED."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max

# d_decision values and the library's numbering of pv::FilterReason (include/trexhip.h)
COMMITTED, BIG, FILTERED, NONE = 0, 1, 16, 255
OUTSIDE_INCLUDE, INSIDE_IGNORE, BDX_IGNORED, OUTSIDE_RANGE, SECOND_THRESHOLD = 0, 1, 2, 3, 4


class Settings:
    def __init__(self, track_threshold=15, method=0, track_threshold_2=0, threshold_ratio_range=(0.5, 1.0), track_size_filter=(), cm_per_pixel=1.0,
                 track_include=(), track_ignore=(), track_ignore_bdx=None):
        self.track_threshold, self.method, self.track_threshold_2 = int(track_threshold), int(method), int(track_threshold_2)
        self.threshold_ratio_range = (F(threshold_ratio_range[0]), F(threshold_ratio_range[1]))
        self.track_size_filter = [(float(a), float(b)) for a, b in track_size_filter]
        self.cm_sqr = F(float(cm_per_pixel) * float(cm_per_pixel))                 # Tracker.cpp:684 (the context's sqcm: double product, narrowed)
        self.track_include = [np.asarray(s, np.float32).reshape(-1, 2) for s in track_include]
        self.track_ignore = [np.asarray(s, np.float32).reshape(-1, 2) for s in track_ignore]
        self.track_ignore_bdx = track_ignore_bdx                                    # per frame: a set of bid words, or None


# ---- core/SizeFilters.cpp -------------------------------------------------------------------------------------------
def max_range(ranges):                                                             # :12-18
    start = end = -1.0
    for a, b in ranges:
        if start == -1 or a < start:
            start = a
        if end == -1 or b > end:
            end = b
    return start, end


def close_to_minimum_of_one(ranges, cmsq, scale_factor):                           # :20-26
    return any(float(cmsq) >= a * float(F(scale_factor)) for a, b in ranges)


def in_range_of_one(ranges, cmsq):                                                 # :36-53 with scale_factor -1
    if not ranges:
        return True
    return any(a <= float(cmsq) < b for a, b in ranges)                            # Range<double>::contains = [start, end)


# ---- UNPINNED commons pieces ------------------------------------------------------------------------------------------
def bounds_of(b):
    return F(b["x0"]), F(b["y0"]), F(int(b["x1"]) - int(b["x0"]) + 1), F(int(b["y1"]) - int(b["y0"]) + 1)


def center_of(b):
    x, y, w, h = bounds_of(b)
    return F(x + F(w * F(0.5))), F(y + F(h * F(0.5)))


def bounds_contains(x, y, w, h, px, py):
    return bool(px >= x and px < F(x + w) and py >= y and py < F(y + h))


def bounds_overlaps(a, b):
    ax, ay, aw, ah = a
    bx, by, bw, bh = b
    return bool(ax < F(bx + bw) and bx < F(ax + aw) and ay < F(by + bh) and by < F(ay + ah))


def pnpoly(pts, tx, ty):                                                           # W. R. Franklin's crossing test
    c = False
    n = len(pts)
    j = n - 1
    for i in range(n):
        xi, yi, xj, yj = F(pts[i][0]), F(pts[i][1]), F(pts[j][0]), F(pts[j][1])
        if (yi > ty) != (yj > ty):
            with np.errstate(all="ignore"):
                cross = F(F(F(F(xj - xi) * F(ty - yi)) / F(yj - yi)) + xi)
            if tx < cross:
                c = not c
        j = i
    return c


# ---- PrefilterBlobs.cpp -------------------------------------------------------------------------------------------------
def blob_matches_shapes(b, shapes):                                                # :328-355
    cx, cy = center_of(b)
    for rect in shapes:
        if len(rect) == 2:
            x, y = F(rect[0][0]), F(rect[0][1])
            if bounds_contains(x, y, F(F(rect[1][0]) - x), F(F(rect[1][1]) - y), cx, cy):
                return True
        elif len(rect) > 2:
            if pnpoly(rect, cx, cy):
                return True
    return False


def rect_overlaps_shapes(bounds, shapes):                                          # :357-385
    for rect in shapes:
        if len(rect) == 2:
            x, y = F(rect[0][0]), F(rect[0][1])
            if bounds_overlaps((x, y, F(F(rect[1][0]) - x), F(F(rect[1][1]) - y)), bounds):
                return True
        elif len(rect) > 2:
            x, y, w, h = F(0), F(0), FLT_MAX, FLT_MAX                              # :364, as written
            for p in rect:                                                         # insert_point
                x, y = min(x, F(p[0])), min(y, F(p[1]))
                w, h = max(w, F(p[0])), max(h, F(p[1]))
            w, h = F(w - x), F(h - y)                                              # :368-369
            if bounds_overlaps((x, y, w, h), bounds):
                return True
    return False


def is_blob_ignored(bid, parent_bid, ignore_set):                                  # :130-150
    if ignore_set is not None:
        if int(bid) in ignore_set or (parent_bid is not None and int(parent_bid) in ignore_set):
            return True
    return False


# ---- pixel counts -----------------------------------------------------------------------------------------------------
def difference(bg, p, method):
    bg, p = bg.astype(np.int32), p.astype(np.int32)
    return np.abs(bg - p) if method == 0 else (np.maximum(bg - p, 0) if method == 1 else p)


def count_at(table, k, bg, method, threshold):
    """Pixels of blob k of a frame table whose difference is >= threshold (pv::Blob::recount before the * cm^2)."""
    b = table.blobs[k]
    runs = table.runs[int(b["run_begin"]):int(b["run_begin"]) + int(b["n_runs"])]
    px = table.pixels[int(b["pix_begin"]):int(b["pix_begin"]) + int(b["n_pixels"])]
    bgv = np.concatenate([bg[int(r["y"]), int(r["x0"]):int(r["x1"]) + 1] for r in runs]) if len(runs) else np.zeros(0, np.uint8)
    return int((difference(bgv, px, method) >= threshold).sum())


# ---- Tracker::prefilter -------------------------------------------------------------------------------------------------
class FrameDecision:
    """det / sub: one d_decision value per detect blob / per sub-blob; order: entries ("det" | "sub", frame-local index), committed first and
    then big, each in the order of the reference's push_back; presumed: per detect blob; second: {entry: pixels at track_threshold_2}."""

    def __init__(self, n1, n2):
        self.det = np.full(n1, NONE, np.uint8)
        self.sub = np.full(n2, NONE, np.uint8)
        self.filtered, self.big = [], []
        self.filtered_out = 0
        self.presumed = np.zeros(n1, np.int32)
        self.second = {}


def prefilter_frame(det, sub, bg, st, frame=0, blob_begin=0):
    """det, sub: the frame's tables of trexhip_fetch and of trexhip_fetch_rethreshold at st.track_threshold; sub parents are
    blob_begin + frame-local detect index."""
    n1, n2 = len(det.blobs), len(sub.blobs)
    out = FrameDecision(n1, n2)
    ranges = st.track_size_filter
    mr_start, mr_end = max_range(ranges)
    cm_sqr = st.cm_sqr
    ignore_set = None
    if st.track_ignore_bdx is not None and st.track_ignore_bdx[frame] is not None:   # :735-740
        ignore_set = set(int(v) for v in st.track_ignore_bdx[frame])
    parents = sub.blobs["parent"].astype(np.int64) - blob_begin

    def filter_out(entry, reason):
        kind, k = entry
        (out.det if kind == "det" else out.sub)[k] = FILTERED + reason
        out.filtered_out += 1

    def table_of(entry):
        return (det if entry[0] == "det" else sub), entry[1]

    def blob_of(entry):
        t, k = table_of(entry)
        return t.blobs[k]

    def parent_bid(entry):
        return None if entry[0] == "det" else det.blobs[int(parents[entry[1]])]["bid"]

    def recount_of(entry):                                                         # :768-774
        t, k = table_of(entry)
        npx = int(t.blobs[k]["n_pixels"])
        full = F(F(npx) * cm_sqr)
        if ranges and float(full) > mr_end * 100:
            return full                                                            # force_set_recount(threshold)
        if entry[0] == "sub":
            return full                                                            # every pixel of a sub-blob survives its own threshold
        survivors = int(sub.blobs["n_pixels"][parents == k].sum())                 # recount(threshold, background)
        return F(F(survivors) * cm_sqr)

    def check_precise_not_ignored(entry):                                          # :742-763
        b = blob_of(entry)
        if st.track_ignore and blob_matches_shapes(b, st.track_ignore):
            filter_out(entry, INSIDE_IGNORE)
            return False
        if st.track_include and not blob_matches_shapes(b, st.track_include):
            filter_out(entry, OUTSIDE_INCLUDE)
            return False
        if is_blob_ignored(b["bid"], parent_bid(entry), ignore_set):
            filter_out(entry, BDX_IGNORED)
            return False
        return True

    def check_blob(entry, precise_check_boundaries):                               # :765-804 (tags / segmentations: not on this path)
        b = blob_of(entry)
        if not precise_check_boundaries:
            if st.track_include and not rect_overlaps_shapes(bounds_of(b), st.track_include):
                filter_out(entry, OUTSIDE_INCLUDE)
                return False
            if is_blob_ignored(b["bid"], parent_bid(entry), ignore_set):
                filter_out(entry, BDX_IGNORED)
                return False
            return True
        return check_precise_not_ignored(entry)

    for j in range(n1):                                                            # :806
        own = ("det", j)
        if not check_blob(own, False):                                             # :816
            continue
        recount = recount_of(own)                                                  # :820
        ptrs = []
        found_blobs = 0
        if (not ranges or close_to_minimum_of_one(ranges, recount, 0.5)) and st.track_threshold > 0:   # :828-831
            pblobs = [("sub", int(i)) for i in np.nonzero(parents == j)[0]]        # threshold_blob: the second table set, table order
            found_blobs = len(pblobs)
            for add in pblobs:                                                     # :841-848
                if not check_blob(add, True):
                    continue
                ptrs.append(add)
        if found_blobs == 0:                                                       # :853-858
            if check_precise_not_ignored(own):
                ptrs.append(own)
            else:
                continue
        for ptr in ptrs:                                                           # :861-914
            recount = recount_of(ptr)
            if in_range_of_one(ranges, recount):
                if st.track_threshold_2 > 0:                                       # :865-874
                    t, k = table_of(ptr)
                    px2 = count_at(t, k, bg, st.method, st.track_threshold_2)
                    out.second[ptr] = px2
                    second_count = F(F(px2) * cm_sqr)
                    lo, hi = F(st.threshold_ratio_range[0] * recount), F(st.threshold_ratio_range[1] * recount)
                    if not (second_count >= lo and second_count < hi):
                        filter_out(ptr, SECOND_THRESHOLD)
                        continue
                (out.det if ptr[0] == "det" else out.sub)[ptr[1]] = COMMITTED      # :908
                out.filtered.append(ptr)
            elif ranges and float(recount) < mr_start:                             # :910-911
                filter_out(ptr, OUTSIDE_RANGE)
            else:                                                                  # :913
                (out.det if ptr[0] == "det" else out.sub)[ptr[1]] = BIG
                out.big.append(ptr)
                out.presumed[j] = 2                                                # split_expectation(2, false), PrefilterBlobs.cpp:223
    return out


def expected_outputs(dets, subs, bg, st, max_batch, max_blobs):
    """The four arrays trexhip_prefilter_device writes for a batch (lists of per-frame tables), plus the second counts."""
    n = len(dets)
    cap, per_frame = max_batch * max_blobs, 2 * max_blobs
    total1 = sum(len(d.blobs) for d in dets)
    decision = np.full(2 * cap, NONE, np.uint8)
    order = np.full((n, per_frame), -1, np.int32)
    counts = np.zeros((n, 4), np.int32)
    presumed = np.zeros(total1, np.int32)
    second = np.full(2 * cap, -1, np.int32)
    for f in range(n):
        d, s = dets[f], subs[f]
        if int(d.info["flags"]) or int(s.info["flags"]):
            counts[f, 3] = 1
            continue
        b1, b2 = int(d.info["blob_begin"]), int(s.info["blob_begin"])
        r = prefilter_frame(d, s, bg, st, f, b1)
        e2, e1 = f * max_blobs, cap + f * max_blobs             # entries are numbered by frame and index in the frame, not by pooled index
        decision[e2:e2 + len(r.sub)] = r.sub
        decision[e1:e1 + len(r.det)] = r.det
        entries = [(e2 + k if kind == "sub" else e1 + k) for kind, k in r.filtered + r.big]
        order[f, :len(entries)] = entries
        counts[f] = (len(r.filtered), len(r.big), r.filtered_out, 0)
        presumed[b1:b1 + len(r.presumed)] = r.presumed
        for (kind, k), v in r.second.items():
            second[e2 + k if kind == "sub" else e1 + k] = v
    return decision, order, counts, presumed, second
