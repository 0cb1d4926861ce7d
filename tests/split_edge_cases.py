"""Constructed scenes for the split search (trexhip_split_search_device, trex_amd/csrc/split.hip) and the table of named cases built from them.
No GPU and no torch: tests/test_split_edge_cases.py holds the table to the oracle alone, tests/test_split_edges_gpu.py holds the device to the oracle.

A "plate and bridge" blob is a stack of rectangles (plates) of chosen size and depth below a flat background, joined by shallower bridges.  Under the
signed difference the bridge disappears at `bridge depth + 1`, so the sizes of the pieces, the splitting threshold and the kernel's size class are
chosen, not found.  Options: a tail row (shorter than its plate, or it would join two plates) for an exact pixel count, a comb (every other column of
some rows as shallow as the bridge) that turns into a chosen number of sub-lines at the splitting threshold, brighter-than-background plates that
only the absolute difference sees, and a diagonal-only contact that holds under connectivity 8 and not under 4.

cm_per_pixel: the reference holds the setting as a float and squares it in float; the library computes (float)(cm * cm) from the double it is given.
For 0.37, 0.1 and 0.0173 the two are one ulp apart unless the double is a widened float, so every non-unit value in this table is
float(np.float32(v)): then cm * cm is exact in double and rounds to the float product.

Every expected value comes from the construction or from float32 / float64 arithmetic restated here (cmsq, the *_edge functions), never from the
code under test."""
import functools
from dataclasses import dataclass, field
import numpy as np
from split_cases import merged_scene

# the kernel's size classes (split.hip): pixels, lines and sub-lines a blob may have in the small, large and huge launch
S_PX_SMALL, S_RUNS_SMALL, S_SUB_SMALL = 2048, 256, 1024
S_PX, S_RUNS, S_SUB = 16384, 1024, 2048
S_PX_HUGE, S_RUNS_HUGE, S_SUB_HUGE = 61440, 2048, 4096
KEEP_ABORT, REMOVE, ABORT, TOO_FEW = 1, 2, 3, 4
BRIDGE = 40                                                  # depth of every bridge unless a case says otherwise: the split is at 41
F32 = np.float32


def f32cm(v):
    return float(F32(v))


def sqcm(cm):
    return F32(cm) * F32(cm)


def cmsq(n, cm):
    """(double)((float)n * sqcm): the size in cm^2 that the search compares with the ranges"""
    return float(F32(n) * sqcm(cm))


def up(v):
    return float(np.nextafter(np.float64(v), np.inf))


def down(v):
    return float(np.nextafter(np.float64(v), -np.inf))


# ---- builders ------------------------------------------------------------------------------------------------------------------------------------------
def comb_gaps(total, kmax):
    """gap counts per comb row that add `total` sub-lines: full rows of kmax, then the remainder"""
    rows = [kmax] * (total // kmax)
    if total % kmax:
        rows.append(total % kmax)
    return rows


def plates_blob(plates, bridge_depth=BRIDGE, bridge=(2, 2), bridge_px=None, diagonal=False, tail_top=None, tail_bottom=0, comb=None, comb_depth=None):
    """-> int16 depth map (frame = background - depth; 0 = background).  plates: (h, w, depth) stacked top to bottom, left-aligned; a negative depth
    is brighter than the background.  bridge: (h, w) rows between consecutive plates, or bridge_px = (n, w): n pixels in rows of w, the last one
    partial.  diagonal: each plate starts where the one above ends, one column to its right, and one bridge pixel below that corner joins them
    4-connected.  tail_top: (n, depth) pixels in a row above the first plate; tail_bottom: n pixels of the last plate's depth below it.
    comb: (plate index, gaps per row from the plate's top): the row's columns 1, 3, .. 2k-1 get comb_depth (default: the bridge's)."""
    rows = []                                                # (x offset, [depths])
    x = 0
    if tail_top:
        assert 0 < tail_top[0] < plates[0][1]
        rows.append((0, [tail_top[1]] * tail_top[0]))
    for i, (h, w, d) in enumerate(plates):
        if i:
            if diagonal:
                x += plates[i - 1][1]
            elif bridge_px:
                n, bw = bridge_px
                while n > 0:
                    rows.append((0, [bridge_depth] * min(n, bw))); n -= bw
            else:
                for _ in range(bridge[0]):
                    rows.append((0, [bridge_depth] * bridge[1]))
        for r in range(h):
            line = [d] * w
            if comb and comb[0] == i and r < len(comb[1]):
                k = comb[1][r]
                assert 2 * k <= w
                for c in range(k):
                    line[2 * c + 1] = bridge_depth if comb_depth is None else comb_depth
            rows.append((x, line))
        if diagonal and i:
            rows[len(rows) - h] = (x - 1, [bridge_depth] + rows[len(rows) - h][1])
    if tail_bottom:
        assert 0 < tail_bottom < plates[-1][1]                # a tail as long as its plate would be one more plate row
        rows.append((x, [plates[-1][2]] * tail_bottom))
    W = max(o + len(l) for o, l in rows)
    out = np.zeros((len(rows), W), np.int16)
    for y, (o, l) in enumerate(rows):
        out[y, o:o + len(l)] = l
    return out


def two_plates_px(total, w, depths=(90, 80)):
    """two plates of width w and a 2 x 2 bridge with exactly `total` pixels: the rows are shared out, the remainder is the tail"""
    body = total - 4
    h = (body - 1) // w
    tail = body - h * w
    if tail == w:
        h, tail = h + 1, 0
    return plates_blob([(h - h // 2, w, depths[0]), (h // 2, w, depths[1])], tail_bottom=tail)


def thin_blob(n_lines, w=4, depths=(90, 80)):
    """tall and thin: two plates of width w and two bridge rows, exactly n_lines lines"""
    h = n_lines - 2
    return plates_blob([(h - h // 2, w, depths[0]), (h // 2, w, depths[1])])


def plate_px(n, w, depth):
    """a plate of exactly n pixels in rows of w -> ((h, w, depth), tail)"""
    return (n // w, w, depth), n % w


def scene(patches, bg=200, shape=None, gap=3):
    """patches side by side on a flat background, `gap` pixels apart, in a frame at least 32 wide -> frame, background, origin (x0, y0) of every patch"""
    H = max(p.shape[0] for p in patches) + 2 * gap
    W = max(sum(p.shape[1] + gap for p in patches) + gap, 32)
    if shape:
        assert shape[0] >= H and shape[1] >= W, (H, W)
        H, W = shape
    img = np.full((H, W), bg, np.int32)
    x, at = gap, []
    for p in patches:
        assert p[0].any() and p[:, 0].any()
        img[gap:gap + p.shape[0], x:x + p.shape[1]] -= p
        at.append((x, gap))
        x += p.shape[1] + gap
    assert img.min() >= 0 and img.max() <= 255
    return img.astype(np.uint8), np.full((H, W), bg, np.uint8), at


# ---- arithmetic restated: on which side of an edge a setting lies ------------------------------------------------------------------------------------
def approx_threshold(begin, max_pixel, keep):
    """threshold_approximate's grid (SplitBlob.cpp:609-706, sequential form) for a blob that is acceptable exactly at keep[0] <= t <= keep[1] and is
    never ABORTed: three interleaved progressions of step 6 over the first 30 % of the thresholds, then of step 3 over the rest"""
    ok = lambda t: keep[0] <= t <= keep[1]
    fs_end = begin + int((max_pixel - begin) * 0.3)
    for ti in range(3):
        for offset in range(2):
            for t in range(begin + ti * 2 + offset, fs_end, 6):
                if ok(t):
                    return t
        for t in range(fs_end + ti, max_pixel, 3):
            if ok(t):
                return t
    return -1


def complete_threshold(begin, max_pixel, keep):
    for t in range(begin, max_pixel):
        if keep[0] <= t <= keep[1]:
            return t
    return -1


def last_start_keeping(n, cm, gs):
    """the largest range start whose removal bound start * (double)(float)gs does not exceed n pixels' size: one ulp more and the piece is removed"""
    x, g = cmsq(n, cm), float(F32(gs))
    lo = x / g
    while lo * g > x:
        lo = down(lo)
    while up(lo) * g <= x:
        lo = up(lo)
    return lo


def last_shrink_keeping(pixels, n, cm):
    """the largest float max_shrink at which a piece of n pixels survives the bound (float)pixels * sqcm * max_shrink of a blob without size ranges"""
    ms = F32(n) / F32(pixels)
    kept = lambda m: not float(F32(n) * sqcm(cm)) < float(F32(pixels) * sqcm(cm) * m)
    while not kept(ms):
        ms = np.nextafter(ms, F32(0))
    while kept(np.nextafter(ms, F32(1))):
        ms = np.nextafter(ms, F32(1))
    return float(ms)


def last_pixels_aborting(first, ms, cm):
    """the largest number of remaining pixels that is still ABORTed after a first size of `first` pixels: (float)r * sqcm < max_shrink * first_size"""
    first_size = F32(first) * sqcm(cm)
    r = int(first * ms) + 2
    while not F32(r) * sqcm(cm) < F32(ms) * first_size:
        r -= 1
    return r


def last_end_guarded(npx, cm):
    """the largest range end at which a blob of npx pixels is not searched at all: (float)npx * sqcm < max_end * 100 fails"""
    x = cmsq(npx, cm)
    hi = x / 100.0
    while x < hi * 100.0:
        hi = down(hi)
    while not x < up(hi) * 100.0:
        hi = up(hi)
    return hi


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Blob:
    """one constructed blob of a case and what the construction says about it"""
    frame: int
    origin: tuple                                            # (x0, y0) of its bounding box
    presumed: int
    outcome: str                                             # found | initial | exhaust | abort | guard | nosearch | capacity | skipped
    threshold: int = -1                                      # the hand-derived SplitBlob threshold; -1 = none
    effective: int = -1
    n_pixels: int = None
    n_runs: int = None
    sublines: int = None                                     # lines of threshold_blob at `sub_at`
    sub_at: int = BRIDGE + 1
    initial_action: int = None
    n_result: int = None
    min_max: tuple = None


@dataclass
class Case:
    name: str
    family: str
    frames: np.ndarray                                       # [n, H, W] as handed to the device
    bg: np.ndarray
    blobs: list                                              # every blob of every frame; None = random scene, every blob presumed `presumed_all`
    method: int = 1
    algorithm: int = 1
    cm: float = 1.0
    ranges: tuple = ()
    detect_kw: dict = field(default_factory=dict)            # detect settings by their shared names (image_invert, connectivity)
    split_kw: dict = field(default_factory=dict)             # trexhip_split_params fields
    edge: tuple = None                                       # (group, side): the oracle's answers differ between the sides of a group
    presumed_all: int = 2
    min_found: int = 0

    @property
    def connectivity(self):
        return self.detect_kw.get("connectivity", 8)

    def oracle_split_kw(self):
        """the keywords of oracle.split_params"""
        k = self.split_kw
        kw = dict(algorithm=self.algorithm, cm_per_pixel=self.cm, size_ranges=list(self.ranges))
        for mine, theirs in (("track_threshold", "track_threshold"), ("track_posture_threshold", "track_posture_threshold"),
                             ("calculate_posture", "calculate_posture"), ("blob_split_max_shrink", "max_shrink"),
                             ("blob_split_global_shrink_limit", "global_shrink_limit")):
            if mine in k:
                kw[theirs] = k[mine]
        return kw


def px_of(patch):
    return int(np.count_nonzero(patch))


def runs_of(patch):
    m = patch != 0
    return int(np.count_nonzero(m[:, 0]) + np.count_nonzero(m[:, 1:] & ~m[:, :-1]))


STD3 = [(8, 12, 90), (8, 12, 80), (8, 12, 70)]               # three pieces of 96 pixels; bridges of 4


def _single(name, family, patch, presumed, outcome, threshold=-1, effective=None, bg=200, invert=False, **kw):
    blob_kw = {k: kw.pop(k) for k in ("n_pixels", "n_runs", "sublines", "sub_at", "initial_action", "n_result", "min_max") if k in kw}
    fr, bgi, at = scene([patch], bg)
    blob_kw.setdefault("n_pixels", px_of(patch)); blob_kw.setdefault("n_runs", runs_of(patch))
    b = Blob(0, at[0], presumed, outcome, threshold, threshold if effective is None else effective, **blob_kw)
    return Case(name, family, (255 - fr if invert else fr)[None], bgi, [b], **kw)


def _family_a(out):
    std = plates_blob(STD3)
    for n, w in ((2048, 32), (2049, 32), (16384, 64), (16385, 64), (61440, 128), (61441, 128)):
        p = two_plates_px(n, w)
        over = n > S_PX_HUGE
        out.append(_single(f"a_pixels_{n}", "a", p, 2, "capacity" if over else "found", -1 if over else 41, n_pixels=n))
    for n in (256, 257, 1024, 1025, 2048, 2049):
        p = thin_blob(n)
        over = n > S_RUNS_HUGE
        c = _single(f"a_lines_{n}", "a", p, 2, "capacity" if over else "found", -1 if over else 41, n_runs=n)
        assert c.blobs[0].n_pixels < S_PX_SMALL or n > 257    # 256 / 257 lines: only the line count decides the class
        out.append(c)
    # one batch that needs all three launches: small, large, huge and beyond-capacity blobs, presumed_nr -1 and 0 among them
    shape = (490, 170)
    large, huge, beyond = two_plates_px(2049, 32), two_plates_px(61440, 128), two_plates_px(61441, 128)
    f0, bg, a0 = scene([std, large, std], shape=shape)
    f1, _, a1 = scene([huge, std], shape=shape)
    f2, _, a2 = scene([beyond, std], shape=shape)
    blobs = [Blob(0, a0[0], 2, "found", 41, 41, n_pixels=296), Blob(0, a0[1], 2, "found", 41, 41, n_pixels=2049), Blob(0, a0[2], 0, "skipped"),
             Blob(1, a1[0], 2, "found", 41, 41, n_pixels=61440), Blob(1, a1[1], -1, "skipped"),
             Blob(2, a2[0], 2, "capacity", n_pixels=61441), Blob(2, a2[1], 3, "found", 41, 41, n_pixels=296)]
    out.append(Case("a_mixed_batch", "a", np.stack([f0, f1, f2]), bg, blobs))


def _family_b(out):
    std = plates_blob(STD3)
    for cls, w, ha, hb, cap in (("large", 64, 100, 88, S_SUB), ("huge", 128, 110, 88, S_SUB_HUGE)):
        for n in (cap, cap + 1):
            p = plates_blob([(ha, w, 90), (hb, w, 80)], comb=(0, comb_gaps(n - ha - hb, (w - 1) // 2)))
            fr, bg, at = scene([p, std])
            over = n > cap
            blobs = [Blob(0, at[0], 2, "capacity" if over else "found", -1 if over else 41, -1 if over else 41, n_pixels=px_of(p), n_runs=ha + hb + 2,
                          sublines=n),
                     Blob(0, at[1], 3, "found", 41, 41, n_pixels=296, n_result=3)]
            assert (S_PX_SMALL < px_of(p) <= S_PX) if cls == "large" else (S_PX < px_of(p) <= S_PX_HUGE)
            out.append(Case(f"b_{cls}_sublines_{n}", "b", fr[None], bg, blobs))
    # the densest comb of the small class: 32 x 64, every other column as shallow as a bridge -> 32 columns of 32 pixels in 1024 one-pixel lines.
    # Without size ranges a piece survives if it has max_shrink of the remaining pixels: 0.02 keeps the 32-pixel columns (1024 * 0.02 = 20.48)
    p = plates_blob([(32, 64, 90)], comb=(0, [32] * 32))
    out.append(_single("b_small_dense_comb", "b", p, 2, "found", 41, n_pixels=S_PX_SMALL, n_runs=32, sublines=S_SUB_SMALL, n_result=32,
                       split_kw=dict(blob_split_max_shrink=0.02)))


def _family_c(out):
    two = plates_blob([(20, 25, 90), (20, 23, 80)])           # 500 and 460 pixels, 964 with the bridge
    for cmv in (0.37, 0.1, 0.0173):
        cm = f32cm(cmv)
        tag = str(cmv).replace("0.", "")
        # the range's lower edge on the smaller piece: cmsq >= start
        x = cmsq(460, cm)
        for side, lo in (("below", down(x)), ("at", x), ("above", up(x))):
            ok = lo <= x
            out.append(_single(f"c_cm{tag}_lower_{side}", "c", two, 2, "found" if ok else "exhaust", 41 if ok else -1, cm=cm, ranges=((lo, cmsq(600, cm)),),
                               initial_action=REMOVE, edge=(f"lower{tag}", "in" if ok else "out")))
        # its upper edge on the larger piece: cmsq < end
        x = cmsq(500, cm)
        for side, hi in (("below", down(x)), ("at", x), ("above", up(x))):
            ok = x < hi
            out.append(_single(f"c_cm{tag}_upper_{side}", "c", two, 2, "found" if ok else "exhaust", 41 if ok else -1, cm=cm, ranges=((cmsq(100, cm), hi),),
                               initial_action=REMOVE, edge=(f"upper{tag}", "in" if ok else "out")))
    cm = f32cm(0.37)
    # cmsq > max_end on the whole blob, presumed_nr = 1: REMOVE / TOO_FEW / KEEP_ABORT as the range's end passes the blob's size
    x = cmsq(964, cm)
    for side, hi, act in (("below", down(x), REMOVE), ("at", x, TOO_FEW), ("above", up(x), KEEP_ABORT)):
        keep = act == KEEP_ABORT
        out.append(_single(f"c_max_end_{side}", "c", two, 1, "initial" if keep else "nosearch", 16 if keep else -1, BRIDGE if keep else -1, cm=cm,
                           ranges=((cmsq(100, cm), hi),), initial_action=act, edge=("max_end", side)))
    # the removal bound max_start * global_shrink on the third piece (100 pixels)
    three = plates_blob([(20, 25, 90), (20, 23, 80), (10, 10, 70)])
    lo = last_start_keeping(100, cm, 5.0)
    for side, s in (("kept", lo), ("removed", up(lo))):
        ok = side == "kept"
        out.append(_single(f"c_bound_shrink5_{side}", "c", three, 3, "found" if ok else "exhaust", 41 if ok else -1, cm=cm, ranges=((s, cmsq(2000, cm)),),
                           split_kw=dict(blob_split_global_shrink_limit=5.0), n_result=3 if ok else None, edge=("bound5", side)))
    cm1 = f32cm(0.1)
    three = plates_blob([(20, 30, 90), (20, 28, 80), (10, 10, 70)])
    lo = last_start_keeping(100, cm1, 0.2)
    assert lo < cmsq(560, cm1)
    for side, s in (("kept", lo), ("removed", up(lo))):
        out.append(_single(f"c_bound_shrink02_{side}", "c", three, 2, "found", 41, cm=cm1, ranges=((s, cmsq(2000, cm1)),),
                           n_result=3 if side == "kept" else 2, edge=("bound02", side)))
    # no size ranges: the bound is (float)pixels * sqcm * max_shrink of the 1200 pixels that remain; the third piece has 240
    cm2 = f32cm(0.0173)
    three = plates_blob([(20, 25, 90), (20, 23, 80), (12, 20, 70)])
    ms = last_shrink_keeping(1200, 240, cm2)
    for side, m in (("kept", ms), ("removed", float(np.nextafter(F32(ms), F32(1))))):
        ok = side == "kept"
        out.append(_single(f"c_bound_noranges_{side}", "c", three, 3, "found" if ok else "exhaust", 41 if ok else -1, cm=cm2,
                           split_kw=dict(blob_split_max_shrink=m), n_result=3 if ok else None, edge=("noranges", side)))
    # ABORT: the pixels that remain at 41 on either side of max_shrink * first_size; 1000 pixels at first, the bridge is the rest
    for ms, w, bw in ((0.05, 5, 30), (0.2, 10, 30), (0.9, 22, 10)):
        r0 = last_pixels_aborting(1000, ms, cm)
        for side, r in (("abort", r0), ("found", r0 + 1)):
            pa, _ = plate_px(r // 2, w, 90)                  # whole rows only; the second plate and its tail take the rest
            pb, tb = plate_px(r - pa[0] * w, w, 80)
            p = plates_blob([pa, pb], bridge_px=(1000 - r, bw), tail_bottom=tb)
            ok = side == "found"
            out.append(_single(f"c_abort_shrink{str(ms).replace('0.', '')}_{side}", "c", p, 2, "found" if ok else "abort", 41 if ok else -1, cm=cm,
                               ranges=((cmsq(10, cm), cmsq(5000, cm)),), split_kw=dict(blob_split_max_shrink=ms), n_pixels=1000,
                               initial_action=TOO_FEW, edge=(f"abort{ms}", side)))
    # the guard (float)npx * sqcm < max_end * 100: 6000 pixels, two pieces of 45 in a bridge of 5910.  The pieces have to lie below max_end, a
    # hundredth of the blob, and 90 pixels survive ABORT only with max_shrink below 90 / 6000: 0.01
    p = plates_blob([(9, 5, 90), (9, 5, 80)], bridge_px=(5910, 60))
    hi = last_end_guarded(6000, cm1)
    for side, e in (("off", hi), ("on", up(hi))):
        ok = side == "on"
        out.append(_single(f"c_guard_{side}", "c", p, 2, "found" if ok else "guard", 41 if ok else -1, cm=cm1, ranges=((cmsq(10, cm1), e),),
                           split_kw=dict(blob_split_max_shrink=0.01), n_pixels=6000, initial_action=REMOVE, edge=("guard", side)))


def _family_d(out):
    low = plates_blob(STD3, tail_top=(5, 20))                 # smallest difference 20: below every initial threshold but the default's
    dark_bright = plates_blob([(8, 12, 90), (8, 12, 80), (8, 12, -70)])
    bright = plates_blob([(8, 12, -180), (8, 12, -170), (8, 12, -160)], bridge_depth=-80)
    diag = plates_blob([(8, 12, 90), (8, 12, 80)], diagonal=True)
    for alg in (1, 2):
        find = complete_threshold if alg == 1 else approx_threshold

        def add(name, patch, presumed, begin, max_pixel, keep, initial=None, bg=200, **kw):
            """begin: the first threshold of the search; keep: the thresholds at which the blob is acceptable; initial: the initial threshold when
            its evaluation is already acceptable"""
            if initial is not None:
                thr, eff, outcome = initial, max(initial, begin), "initial"
            else:
                thr = find(begin, max_pixel, keep) if keep else -1
                eff, outcome = thr, "found" if thr >= 0 else "exhaust"
            out.append(_single(f"d_{name}_alg{alg}", "d", patch, presumed, outcome, thr, eff, bg=bg, algorithm=alg, **kw))

        add("posture30_on", low, 3, 31, 90, (41, 70), split_kw=dict(track_posture_threshold=30, calculate_posture=1))
        add("posture30_off", low, 3, 20, 90, (41, 70), split_kw=dict(track_posture_threshold=30, calculate_posture=0))
        add("posture50_on", low, 3, 51, 90, (41, 70), initial=51, split_kw=dict(track_posture_threshold=50, calculate_posture=1), initial_action=KEEP_ABORT)
        add("posture50_off", low, 3, 20, 90, (41, 70), split_kw=dict(track_posture_threshold=50, calculate_posture=0))
        add("track_above_bridge", low, 3, 46, 90, (41, 70), initial=46, split_kw=dict(track_threshold=45), initial_action=KEEP_ABORT)
        add("track_above_plates", low, 3, 96, 90, None, split_kw=dict(track_threshold=95), initial_action=TOO_FEW)
        # two dark plates and a bright one on 150: the absolute difference sees three pieces, the signed one two, the grey values (60, 70, bridges
        # 110, bright plate 220) never two pieces that both survive the removal bound
        add("dark_bright_absolute", dark_bright, 3, 40, 90, (41, 70), bg=150, method=0)
        add("dark_bright_signed", dark_bright, 3, 16, 90, None, bg=150, method=1, min_max=(0, 90))
        add("dark_bright_signed_two", dark_bright, 2, 16, 90, (41, 80), bg=150, method=1)
        add("dark_bright_none", dark_bright, 2, 60, 220, None, bg=150, method=2, min_max=(60, 220))
        # bright plates (200, 190, 180; bridges 100) on 20
        add("bright_absolute", bright, 3, 80, 180, (81, 160), bg=20, method=0)
        add("bright_signed", bright, 3, 16, 0, None, bg=20, method=1, min_max=(0, 0), initial_action=TOO_FEW)
        add("bright_none", bright, 3, 100, 200, (101, 180), bg=20, method=2)
        add("image_invert", low, 3, 20, 90, (41, 70), invert=True, detect_kw=dict(image_invert=1))
        add("diagonal_connectivity8", diag, 2, 40, 90, None)
        add("diagonal_connectivity4", diag, 2, 40, 90, (41, 80), detect_kw=dict(connectivity=4))
        for span in (0, 1, 3, 4):                             # max_pixel - begin: the approximate search's 30 % segment is empty or one wide
            d = BRIDGE + span
            add(f"span{span}", plates_blob([(8, 12, d), (8, 12, d)]), 2, BRIDGE, d, (41, d) if span else None, min_max=(BRIDGE, d))


def _family_e(out):
    std = plates_blob(STD3)
    # every difference 255: grey value 0 on 255, which the detect pass only keeps with zero_is_background off.  min_pixel starts at 254 (:142)
    full, keep0 = plates_blob([(8, 12, 255)]), dict(zero_is_background=0)
    out.append(_single("e_all255_one", "e", full, 1, "initial", 16, 254, bg=255, min_max=(254, 255), initial_action=KEEP_ABORT, detect_kw=keep0))
    out.append(_single("e_all255_two", "e", full, 2, "exhaust", bg=255, min_max=(254, 255), initial_action=TOO_FEW, detect_kw=keep0))
    out.append(_single("e_flat", "e", plates_blob([(8, 12, 90)]), 2, "exhaust", min_max=(90, 90)))
    # one shallow pixel in front: 21 .. 89 are one pixel set, evaluated once
    out.append(_single("e_flat_low_pixel", "e", plates_blob([(8, 12, 90)], tail_top=(1, 20)), 2, "exhaust", min_max=(20, 90)))
    out.append(_single("e_min_pixel_above_initial", "e", plates_blob(STD3[:2]), 1, "initial", 16, BRIDGE, min_max=(BRIDGE, 90), initial_action=KEEP_ABORT))
    for pn, outcome, thr, eff in ((1, "initial", 16, BRIDGE), (2, "found", 41, 41), (3, "found", 41, 41), (4, "exhaust", -1, -1), (1 << 20, "exhaust", -1, -1)):
        out.append(_single(f"e_presumed_{pn}", "e", std, pn, outcome, thr, eff, n_result=3 if outcome == "found" else None))
    out.append(_single("e_presumed_2_alg2", "e", std, 2, "found", approx_threshold(BRIDGE, 90, (41, 80)), algorithm=2))
    out.append(_single("e_presumed_3_alg2", "e", std, 3, "found", approx_threshold(BRIDGE, 90, (41, 70)), algorithm=2, n_result=3))


def _family_f(out):
    cm = f32cm(0.37)
    s = float(sqcm(cm))
    for alg in (1, 2):
        frames = []
        for seed in range(4):
            fr, bg, _ = merged_scene(70 + seed + 10 * alg)
            frames.append(fr)
        out.append(Case(f"f_merged_cm37_alg{alg}", "f", np.stack(frames), bg, None, algorithm=alg, cm=cm, ranges=((40 * s, 330 * s),), min_found=3))


@functools.lru_cache(maxsize=None)
def table():
    """name -> Case; built once, leave unchanged"""
    out = []
    for fam in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f):
        fam(out)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


NAMES = sorted(table())
