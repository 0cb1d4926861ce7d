"""Scenes shared by the detect tests (tests/test_segment_gpu.py) and the track-stage tests behind every labelling path
(tests/test_rethreshold_paths_gpu.py): which path of launch_segment labels a frame follows from its line count, so the scenes are made here once,
with the conditions each one has to meet (checked from the oracle's tables, on the CPU: tests/test_ccl_scenes.py, and again by the GPU tests)."""
import functools
import numpy as np
from oracle import oracle
from trex_amd import synth

BLOB_BELOW_RANGE, BLOB_BIG = 1, 2                                   # TREXHIP_BLOB_* of include/trexhip.h
TRACK_PAIRS = ((0, 60), (1, 40), (2, 50))                           # (method, threshold): absolute, signed and no difference
TRACK_RANGES = [(3, 50)]


def ladder_frames():
    """six 128 x 128 frames on a flat background: two light (under 2000 lines), two medium (2001 .. 3840), two heavy (3841 .. 8160); noise of
    many small blobs beside structured frames whose lines all belong to a few large blobs"""
    rng = np.random.default_rng(2000)
    W = H = 128
    bg = np.full((H, W), 120, np.uint8)
    def noise(density):
        f = bg.copy(); f[rng.random((H, W)) < density] = 10
        return f
    light = bg.copy()                                                # a few solid blobs, one of them through most rows
    light[5:120, 10:14] = 10; light[30:40, 40:90] = 10; light[60:100:2, 20:120] = 10; light[110:125, 100:127] = 10
    medium = bg.copy()                                               # 24 lines in every row, joined by a bar every 16 rows: few blobs of many lines
    for j in range(24): medium[:, 2 + 5 * j:2 + 5 * j + 1 + j % 4] = 10
    medium[::16, :] = 10
    heavy = bg.copy()                                                # lines of two pixels, one apart, shifted row by row: ONE 8-connected blob of ~5.4 k lines
    ys, xs = np.mgrid[0:H, 0:W]
    heavy[(xs + ys) % 3 != 0] = 10
    return bg, [noise(0.05), light], [noise(0.2), medium], [noise(0.5), heavy]


def textured(frames, bg, seed=7):
    """the same masks, every foreground pixel drawn from 1 .. 105: on a flat background of 120 the detect pass at its default threshold of 15
    sees exactly the same lines (difference 15 .. 119, no zero pixel), and a track threshold cuts them into sub-runs"""
    assert np.all(bg == 120)
    rng = np.random.default_rng(seed)
    out = []
    for f in frames:
        g = f.copy()
        m = f != bg
        g[m] = rng.integers(1, 106, int(m.sum()))
        out.append(g)
    return out


LADDER_CAPS = dict(max_runs=8000, max_blobs=4096, max_pixels=128 * 128)
LADDER_BRACKET = [(0, 1999)] * 2 + [(2001, 3840)] * 2 + [(3841, 8160)] * 2     # light, medium, heavy: what the S, the M and the L instance hold


@functools.lru_cache(maxsize=None)
def textured_ladder():
    """-> bg, the six distinct frames of ladder_frames() textured: [noise, structured] x [light, medium, heavy]"""
    bg, light, medium, heavy = ladder_frames()
    return bg, textured(light + medium + heavy, bg)


def band_frames(rng, W=1024, H=2048):
    """the frames of the banded detect test: tall columns and a staircase through every seam, ~6000 lines of noise, ~16000 lines (the global chain:
    the band workgroups leave it alone), a bar on the middle seam over single-line blobs, ~5000 lines inside one band of rows (more than a band
    workgroup takes), and an empty frame -> bg, frames"""
    bg = np.full((H, W), 120, np.uint8)
    frames = []
    f = bg.copy()                                                    # tall columns and diagonals through every seam
    for x in range(20, 1000, 480):
        f[int(rng.integers(0, 400)):int(rng.integers(1500, H)), x:x + int(rng.integers(1, 9))] = 10
    for k in range(0, 400):
        f[300 + k * 2:300 + k * 2 + 3, 40 + k:40 + k + 2] = 10       # a staircase: 8-connected only through its corners in places
    frames.append(f)
    f, _ = synth.random_scene(rng, W, H, density=0.018); frames.append(f)        # ~6000 lines: labelled in LDS, banded
    f, _ = synth.random_scene(rng, W, H, density=0.05); frames.append(f)         # ~16000 lines: the global-memory chain (the band workgroups leave it alone)
    f = bg.copy(); f[H // 2 - 3:H // 2 + 3, :] = 10; f[::2, 5:9] = 10; frames.append(f)       # a bar on the middle seam, single-line blobs everywhere
    f = bg.copy()                                                    # ~5000 lines inside ONE band of rows: the band workgroup cannot hold them
    for y in range(0, 250):
        for j in range(20):
            f[y, 10 + 50 * j:10 + 50 * j + 3 + (y % 7)] = 10
    frames.append(f)
    frames.append(bg.copy())                                         # an empty frame
    return bg, frames


BAND_CAPS = dict(max_runs=20000, max_blobs=16384, max_pixels=1 << 21)
CCL_NMAX = 8160                                                      # lines of a frame k_ccl_lds holds; more go to the global-memory chain


@functools.lru_cache(maxsize=None)
def textured_band_frames():
    """-> bg, the banded scenes textured, without the ~16000-line frame (global_chain_frames() has one like it)"""
    bg, frames = band_frames(np.random.default_rng(102))
    del frames[2]
    return bg, textured(frames, bg)


@functools.lru_cache(maxsize=None)
def odd_height_frame():
    """640 x 1000, ~4000 textured lines: the last band is shorter than the others"""
    fr, bg = synth.random_scene(np.random.default_rng(103), 640, 1000, density=0.04)
    return bg, textured([fr], bg)[0]


@functools.lru_cache(maxsize=None)
def global_chain_frames():
    """-> bg, [more than 8160 lines (launch_pending's k_rowscan / k_link / k_flatten / k_blobs), a frame k_ccl_lds holds, an empty one]; random_scene
    draws its bars from 0 .. 89 on 120, so the frames are textured as they come"""
    rng = np.random.default_rng(104)
    W, H = 1024, 1280
    heavy, bg = synth.random_scene(rng, W, H, density=0.05)
    small, _ = synth.random_scene(rng, W, H, density=0.01)
    return bg, [heavy, small, bg.copy()]


def pass2_overflow_frame():
    """256 x 64: 56 detect lines of 240 pixels whose every other pixel fails |bg - p| >= 150 -> 120 sub-runs per line, 6720 in all"""
    bg = np.full((64, 256), 200, np.uint8)
    f = bg.copy()
    f[4:60, 8:248] = 100
    f[4:60, 8:248:2] = 20
    return bg, f


OVERFLOW_MAX_RUNS = 4096


def pass2_many_blobs_frame():
    """256 x 64: eight detect blocks (difference 50) studded with isolated dark pixels (difference 180), two apart both ways: at threshold 150 each of
    them is a sub-blob of its own, 2304 out of 8 detect blobs"""
    bg = np.full((64, 256), 200, np.uint8)
    f = bg.copy()
    for j in range(8):
        x = 4 + 31 * j
        f[8:56, x:x + 25] = 150
        f[9:56:2, x + 1:x + 25:2] = 20
    return bg, f


MANY_BLOBS_MAX_BLOBS = 512


def settings_scene():
    """512 x 64, textured background and frame: detect blobs of every size whose interiors straddle a track threshold (with image_invert the
    device is handed 255 - frame, so that the inverted image is this scene)"""
    rng = np.random.default_rng(12)
    W, H = 512, 64
    bg = rng.integers(90, 170, (H, W)).astype(np.uint8)
    fr = np.clip(bg.astype(int) + rng.integers(-10, 10, (H, W)), 0, 255).astype(np.uint8)
    for _ in range(40):
        y, x = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 30))
        h, w = int(rng.integers(1, 12)), int(rng.integers(1, 30))
        sign = 1 if rng.random() < 0.3 else -1                       # brighter blobs too: the signed difference drops them
        fr[y:y + h, x:x + w] = np.clip(bg[y:y + h, x:x + w].astype(int) + sign * rng.integers(5, 85, (h, w)), 1, 255)
    return bg, fr


SETTINGS_CASES = {
    "connectivity4": dict(connectivity=4),
    "image_invert": dict(image_invert=1),
    "size_filter": dict(size_ranges=[(50, 100000)]),                 # drops the smaller half of the detect blobs: blob_map == -1 for their lines
    "threshold_maximum": dict(threshold_maximum=60),
    "signed_difference": dict(absolute_difference=0),
}


def wide_frames(W, n, H=32):
    """n frames of H rows at width W on a textured background: textured lines across x = 2047 / 2048 (where the row is that wide), one that ends with
    the row, one in the last column"""
    rng = np.random.default_rng(W * 31 + n)
    bg = rng.integers(100, 160, (H, W)).astype(np.uint8)
    frames = []
    for i in range(n):
        fr = np.clip(bg.astype(int) + rng.integers(-8, 8, (H, W)), 0, 255).astype(np.uint8)
        def draw(y, x0, x1):
            x0, x1 = max(x0, 0), min(x1, W)
            if x1 > x0: fr[y % H, x0:x1] = np.clip(bg[y % H, x0:x1].astype(int) - rng.integers(20, 90, x1 - x0), 1, 255)      # a solid detect line, textured
        for _ in range(12):
            x = int(rng.integers(0, W)); draw(int(rng.integers(0, H)), x, x + int(rng.integers(1, 40)))
        for _ in range(3):                                                          # blobs of several rows
            x, y, w = int(rng.integers(0, W)), int(rng.integers(0, H - 4)), int(rng.integers(2, 30))
            for dy in range(4): draw(y + dy, x + dy, x + dy + w)
        draw(i, 2040, 2060); draw(i + 1, 2030, 2048); draw(i + 2, 2048, 2070)      # across, up to and from the chunk border
        draw(i + 5, W - 9, W)                                                       # ends with the row
        draw(i + 7, 0, 6)
        fr[(i + 9) % H, W - 1] = 1
        frames.append(fr)
    return bg, frames


# ---- the oracle's tables, computed once per process ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables(key, method, thr, ranges, detect_kw):
    bg, frame = _FRAMES[key]
    kw = dict(detect_kw)
    H, W = frame.shape
    return oracle.rethreshold_frame(frame, bg, oracle.make_params(W, H, **kw), method, thr, list(ranges), invert=bool(kw.get("image_invert", 0)))


@functools.lru_cache(maxsize=None)
def _detect(key, detect_kw):
    bg, frame = _FRAMES[key]
    H, W = frame.shape
    return oracle.segment(frame, bg, oracle.make_params(W, H, **dict(detect_kw)))


_FRAMES = {}


def _freeze(kw):
    return tuple(sorted((k, tuple(map(tuple, v)) if isinstance(v, list) else v) for k, v in kw.items()))


def register(key, bg, frame):
    """name a frame, so that its oracle tables are computed once and shared by the tests that need them"""
    _FRAMES.setdefault(key, (bg, frame))
    return key


def detect_tables(key, **detect_kw):
    """oracle.segment of a registered frame -> (blobs, runs, pixels); shared, leave unchanged"""
    return _detect(key, _freeze(detect_kw))


def sub_tables(key, method, thr, ranges=(), **detect_kw):
    """oracle.rethreshold_frame of a registered frame -> (blobs, runs, pixels); shared, leave unchanged"""
    return _tables(key, method, thr, tuple(map(tuple, ranges)), _freeze(detect_kw))


def check_capacities(key, caps, pairs=TRACK_PAIRS, ranges=TRACK_RANGES, **detect_kw):
    """the frame's detect tables and its sub-blob tables at every (method, threshold) fit the context's per-frame capacities"""
    db, dr, dp = detect_tables(key, **detect_kw)
    assert len(dr) <= caps["max_runs"] and len(db) <= caps["max_blobs"] and len(dp) <= caps["max_pixels"], (key, len(dr), len(db), len(dp))
    for method, thr in pairs:
        ob, orr, opx = sub_tables(key, method, thr, ranges, **detect_kw)
        assert 0 < len(orr) <= caps["max_runs"], (key, method, thr, len(orr))
        assert len(ob) <= caps["max_blobs"] and len(opx) <= caps["max_pixels"], (key, method, thr, len(ob), len(opx))


def check_ladder():
    """every textured ladder frame keeps its detect bracket and fits the capacities at every pair; the structured frames show all three size classes"""
    bg, distinct = textured_ladder()
    plain = sum(ladder_frames()[1:], [])
    for k, f in enumerate(distinct):
        key = register(("ladder", k), bg, f)
        lo, hi = LADDER_BRACKET[k]
        n_lines = len(detect_tables(key)[1])
        assert lo <= n_lines <= hi, (k, n_lines)
        assert n_lines == len(oracle.segment(plain[k], bg, oracle.make_params(128, 128))[1])        # the texture moved no line
        check_capacities(key, LADDER_CAPS)
    classes = set()
    for k in (1, 3, 5):
        for method, thr in TRACK_PAIRS:
            classes |= set(sub_tables(("ladder", k), method, thr, TRACK_RANGES)[0]["flags"].tolist())
    assert classes == {0, BLOB_BELOW_RANGE, BLOB_BIG}, classes


def check_pass2_overflow():
    """n_raw_runs <= max_runs < n2 <= 2 * max_runs: the detect pass takes the frame, pass 2 cannot, and what an unguarded k_sub would spill stays
    inside one further frame's share"""
    bg, f = pass2_overflow_frame()
    key = register("pass2_overflow", bg, f)
    n1 = len(detect_tables(key)[1])
    n2 = len(sub_tables(key, 0, 150)[1])
    assert (n1, n2) == (56, 6720)
    assert n1 <= OVERFLOW_MAX_RUNS < n2 <= 2 * OVERFLOW_MAX_RUNS
    assert 0 < len(sub_tables(key, 0, 60)[1]) <= OVERFLOW_MAX_RUNS        # ... and at threshold 60 it fits


def check_pass2_many_blobs():
    """the detect blobs and every run count fit; only pass 2's blobs exceed max_blobs"""
    bg, f = pass2_many_blobs_frame()
    key = register("pass2_many_blobs", bg, f)
    db, dr, dp = detect_tables(key)
    ob, orr, opx = sub_tables(key, 0, 150)
    assert len(db) == 8 and len(ob) == 2304 and np.all(ob["n_pixels"] == 1)
    assert len(db) <= MANY_BLOBS_MAX_BLOBS < len(ob) and len(dr) <= 8000 and len(orr) <= 8000 and len(dp) <= 256 * 64


PER_BLOB_FRAMES = (3, 5, 0)                                          # of textured_ladder(): medium and heavy structured, light noise


def per_blob_thresholds(n_blobs):
    """one threshold per detect blob of a frame, every fifth blob left out"""
    return np.array([-1 if k % 5 == 4 else 25 + 6 * (k % 12) for k in range(n_blobs)], np.int32)


def check_per_blob_scene(method):
    """a blob of thousands of lines in each structured frame, hundreds of blobs in the noise frame, and no two sub-blobs of a parent with one bid (they
    are matched by it) -> the thresholds per frame, the size ranges"""
    bg, distinct = textured_ladder()
    thresholds, most_lines, n_blobs = [], [], []
    for k in PER_BLOB_FRAMES:
        db, dr, dp = detect_tables(register(("ladder", k), bg, distinct[k]))
        thr = per_blob_thresholds(len(db))
        for j, b in enumerate(db):
            if thr[j] >= 0:
                ob, _, _ = oracle.threshold_blob(dr[b["run_begin"]:b["run_begin"] + b["n_runs"]], dp[b["pix_begin"]:b["pix_begin"] + b["n_pixels"]],
                                                 bg, method, int(thr[j]))
                assert len(set(ob["bid"].tolist())) == len(ob), (k, j)
        thresholds.append(thr); most_lines.append(int(db["n_runs"].max())); n_blobs.append(len(db))
    assert most_lines[0] > 1000 and most_lines[1] > 4000 and n_blobs[2] > 300, (most_lines, n_blobs)
    assert thresholds[0][0] >= 0 and thresholds[1][0] >= 0             # the large blobs are not among the ones left out
    return thresholds, TRACK_RANGES
