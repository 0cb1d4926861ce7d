"""CPU checks of the normalised-crop oracle (FilterCache.cpp:21-115,276-288): the fixed-point warp against scipy's float
bilinear interpolation, and the transform composition against a direct numpy restatement."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import oracle


def _smooth(h, w, seed):
    rng = np.random.default_rng(seed)
    img = ndimage.gaussian_filter(rng.uniform(0, 255, (h, w)), 3.0)
    img = (img - img.min()) / (img.max() - img.min()) * 255
    return img.astype(np.uint8)


# (matrix, output size (w, h), source size (h, w)): the 80 x 80 crop, then the output sizes of test_crops_sizes_gpu.py, each with a map that
# keeps most of the output inside a 150 x 170 source (non-square outputs: a row / column mix-up of the fixed-point terms shows here)
WARP_CASES = [
    ([1, 0, 3.25, 0, 1, -2.5], (80, 80), (90, 110)),
    ([0.8660254, -0.5, 20.0, 0.5, 0.8660254, -10.0], (80, 80), (90, 110)),
    ([1.2, 0.3, -4.0, -0.2, 0.9, 12.0], (80, 80), (90, 110)),
    ([0.866, -0.5, 20, 0.5, 0.866, -10], (96, 40), (150, 170)),
    ([0.1, 0.02, 1, -0.02, 0.1, 2], (16, 16), (150, 170)),
    ([1.5, 0.4, -30, -0.4, 1.5, 60], (256, 256), (150, 170)),
    ([1.9, 0, 3.3, 0, 0.1, 0.7], (320, 16), (150, 170)),
]


@pytest.mark.parametrize("M,size,src_shape", WARP_CASES, ids=["M0", "M1", "M2", "96x40", "16x16", "256x256", "320x16"])
def test_warp_matches_float_bilinear_within_quantisation(M, size, src_shape):
    OW, OH = size
    src = _smooth(src_shape[0], src_shape[1], 1)
    M = np.asarray(M, np.float32)
    got = oracle.warp_affine(src, M, OW, OH)
    assert got.shape == (OH, OW)
    A = np.array([[M[0], M[1]], [M[3], M[4]]], np.float64)
    Ainv = np.linalg.inv(A)
    off = -Ainv @ np.array([M[2], M[5]], np.float64)
    # scipy works in (row, col): swap axes of the inverse map
    P = np.array([[Ainv[1, 1], Ainv[1, 0]], [Ainv[0, 1], Ainv[0, 0]]])
    want = ndimage.affine_transform(src.astype(np.float64), P, offset=[off[1], off[0]], output_shape=(OH, OW), order=1, mode="constant", cval=0)
    # interior only: border pixels blend with the constant 0 differently at the 1/32 fraction grid
    yy, xx = np.mgrid[0:OH, 0:OW]
    sx = Ainv[0, 0] * xx + Ainv[0, 1] * yy + off[0]
    sy = Ainv[1, 0] * xx + Ainv[1, 1] * yy + off[1]
    inner = (sx > 1) & (sx < src.shape[1] - 2) & (sy > 1) & (sy < src.shape[0] - 2)
    assert inner.sum() > min(1000, OW * OH // 2)
    d = np.abs(got.astype(np.float64) - want)[inner]
    print(size, "inner", int(inner.sum()), "max", d.max(), "mean", d.mean())
    assert d.max() <= 1.0 and d.mean() < 0.4


def test_identity_warp_is_a_copy_with_zero_border():
    src = _smooth(40, 50, 2)
    got = oracle.warp_affine(src, np.array([1, 0, 0, 0, 1, 0], np.float32), 80, 80)
    assert np.array_equal(got[:40, :50], src)
    assert got[40:].sum() == 0 and got[:, 50:].sum() == 0


def test_normalize_transform_composition():
    # t = translate(size/2) . scale(s) . translate(len*0.4 | (-len/2, 0)) . tr      (FilterCache.cpp:50-63)
    tr = np.array([0.6, -0.8, 5.0, 0.8, 0.6, -7.0], np.float32)

    def H(m):
        return np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0, 0, 1]], np.float64)

    for legacy in (False, True):
        ln, s = 30.0, 0.5
        T1 = H([1, 0, 40, 0, 1, 40]); S = H([s, 0, 0, 0, s, 0])
        T2 = H([1, 0, -ln / 2, 0, 1, 0]) if legacy else H([1, 0, ln * 0.4, 0, 1, ln * 0.4])
        want = (T1 @ S @ T2 @ H(tr))[:2].reshape(-1)
        got = oracle.normalize_transform(tr, ln, legacy, 80, 80, s)
        assert np.allclose(got, want, atol=1e-4)


def test_nearest_warp_picks_source_pixels():
    # INTER_NEAREST (r3g3b2 crops): every output is a source pixel or the border value, identity is a copy
    src = _smooth(50, 60, 3)
    M = np.array([0.8, -0.6, 25.0, 0.6, 0.8, -5.0], np.float32)
    got = np.zeros((80, 80), np.uint8)
    oracle.lib().oracle_warp_affine_nearest_u8(oracle._ptr(np.ascontiguousarray(src)), 60, 50, oracle._ptr(M), oracle._ptr(got), 80, 80)
    A = np.array([[M[0], M[1]], [M[3], M[4]]], np.float64); Ainv = np.linalg.inv(A); off = -Ainv @ np.array([M[2], M[5]], np.float64)
    yy, xx = np.mgrid[0:80, 0:80]
    sx = np.rint(Ainv[0, 0] * xx + Ainv[0, 1] * yy + off[0]).astype(int); sy = np.rint(Ainv[1, 0] * xx + Ainv[1, 1] * yy + off[1]).astype(int)
    inside = (sx >= 0) & (sx < 60) & (sy >= 0) & (sy < 50)
    want = np.where(inside, src[np.clip(sy, 0, 49), np.clip(sx, 0, 59)], 0)
    assert (got != want).mean() < 0.02                      # only ties of the rounding at the 1/1024 grid may differ
    ident = np.zeros((50, 60), np.uint8)
    oracle.lib().oracle_warp_affine_nearest_u8(oracle._ptr(np.ascontiguousarray(src)), 60, 50, oracle._ptr(np.array([1, 0, 0, 0, 1, 0], np.float32)), oracle._ptr(ident), 60, 50)
    assert np.array_equal(ident, src)


# ---- the shared crop scene (tests/crop_scenes.py): every blob class has to be what the device tests take it for ----
def test_crop_scene_holds_every_blob_class():
    import crop_scenes as cs
    fr, bg = cs.gray()
    frc, bgc = cs.bgr()
    assert fr.shape == (3, cs.H, cs.W) and frc.shape == (3, cs.H, cs.W, 3) and (cs.W, cs.H) == (320, 1100)
    assert len(np.unique(bg)) > 16 and all(len(np.unique(bgc[..., c])) > 16 for c in range(3))       # textured backgrounds
    p = oracle.make_params(cs.W, cs.H)
    found = {}
    for f in range(3):
        blobs, runs, _ = oracle.segment(fr[f], bg, p)
        b2, r2, _ = oracle.segment(oracle.bgr2gray(frc[f]), oracle.bgr2gray(bgc), p)
        assert runs.tobytes() == r2.tobytes() and np.array_equal(blobs["n_runs"], b2["n_runs"])      # BGR variant: the same geometry
        bi, ri, _ = oracle.segment(255 - fr[f], bg, oracle.make_params(cs.W, cs.H, image_invert=1))
        assert runs.tobytes() == ri.tobytes()                                                         # and the inverted frames under image_invert
        names = cs.classify(f, blobs)
        assert sorted(names) == sorted(n for n, (ff, *_r) in cs.BOXES.items() if ff == f), (f, names)
        assert len(blobs) == len(names)
        for name, k in names.items():
            b = blobs[k]
            rs = runs[int(b["run_begin"]):int(b["run_begin"]) + int(b["n_runs"])]
            mask = np.zeros((cs.H, cs.W), bool)
            for q in rs:
                mask[int(q["y"]), int(q["x0"]):int(q["x1"]) + 1] = True
            assert np.array_equal(mask, cs.masks()[f] & mask) and mask.sum() == b["n_pixels"]
            px = fr[f][mask].astype(int); bgv = bg[mask].astype(int)
            assert len(np.unique(px)) > 32                                                            # pixels are no constants
            assert (px > bgv).mean() > 0.1 and (px < bgv).mean() > 0.5                                # difference 1 != difference 2
            w, h = int(b["x1"]) - int(b["x0"]) + 1, int(b["y1"]) - int(b["y0"]) + 1
            found[name] = dict(lines=int(b["n_runs"]), rows=h, w=w, box=w * h, x0=int(b["x0"]), y0=int(b["y0"]), mask=mask)
    assert sorted(found) == list("abcdefgh")
    small = [n for n in found if found[n]["lines"] <= cs.W_NR and found[n]["rows"] <= cs.W_ROWS]
    assert sorted(small) == list("abcdeg")
    a, b, c, d, e, f_, g, h = (found[n] for n in "abcdefgh")
    assert a["box"] * 3 <= cs.W_IMG                                   # a: painted into LDS even as rgb8 (box <= 5461)
    assert b["box"] <= cs.W_IMG < b["box"] * 3 and 80 <= b["w"] <= 100 and 80 <= b["rows"] <= 100
    assert c["box"] > cs.W_IMG and 140 <= c["w"] <= 160 and 170 <= c["rows"] <= 190
    box = c["mask"][c["y0"]:c["y0"] + c["rows"], c["x0"]:c["x0"] + c["w"]]
    hole = ndimage.binary_fill_holes(box) & ~box                      # c: enclosed background of at least 40 x 40
    ys, xs = np.nonzero(hole)
    assert hole.sum() >= 40 * 40 and np.ptp(ys) + 1 >= 40 and np.ptp(xs) + 1 >= 40 and hole[ys.min():ys.max() + 1, xs.min():xs.max() + 1].all()
    assert d["w"] > 256 and d["rows"] == 7 and d["x0"] == 0 and d["y0"] == 0
    assert e["rows"] == cs.W_ROWS and e["lines"] <= cs.W_NR           # at the row limit
    assert f_["rows"] == 1040 and f_["lines"] <= cs.W_NR              # over the row limit only
    assert 2040 <= g["lines"] <= cs.W_NR and g["rows"] <= cs.W_ROWS   # at the line limit
    assert h["lines"] >= 2500 and h["rows"] <= cs.W_ROWS              # over the line limit only
    assert f_["box"] <= cs.W_IMG < h["box"]                           # the two over-limit blobs: one painted into LDS, one with per-tap line tests
    # the oracle crops of the over-limit blobs are not empty at any tested output size
    for f, name in ((1, "f"), (2, "h")):
        blobs, runs, _ = oracle.segment(fr[f], bg, p)
        k = cs.classify(f, blobs)[name]
        for ow, oh in cs.SIZES:
            want, _ = oracle.crop_normalized(fr[f], bg, blobs[k], runs, out_w=ow, out_h=oh)
            assert want.any(), (name, ow, oh)
