"""The device crops (k_crops_none, k_warp_maps + k_crops_warp) against the oracle at every output size and blob extreme: bit for bit.

The scene (tests/crop_scenes.py, its blob classes pinned by test_crops_oracle.py) holds one blob per path of crops.hip: painted into
LDS or tested per tap (per encoding), with a hole, cut and padded at once, at and beyond the LDS line tables (1024 rows, 2048 lines).
Every launch crops every blob a..h of the three frames; the list below is a pairwise cover of
  output size x entry point x difference x scale x encoding, not their product.
Every buffer is filled with 77 and holds one crop more than the call is asked for: the extra crop has to stay 77."""
import numpy as np
import pytest
import torch

import crop_scenes as cs
from oracle import oracle
from trex_amd import capi

pytestmark = pytest.mark.gpu

MP = 1024
SENTINEL = 77
E_INVALID = -1            # TREXHIP_E_INVALID (include/trexhip.h)


class Scene:
    """one encoding: the segmented batch on its context, the host images the oracle reads (one per channel), midline poses"""
    def __init__(self, enc, invert=False):
        self.enc, self.invert = enc, invert
        kw = dict(max_batch=cs.N_FRAMES, pixel_encoding=enc, image_invert=1 if invert else 0)
        self.seg = seg = capi.Segmenter(capi.default_params(cs.W, cs.H, **kw))
        if enc == capi.ENC_GRAY:
            fr, bg = cs.gray()
            seg.set_background(bg)
            self.d_frames = torch.from_numpy(255 - fr if invert else fr).cuda()
            seg.segment_device(self.d_frames.data_ptr(), cs.N_FRAMES)
            self.planes, self.bgs, gray_fr, gray_bg = [255 - fr if invert else fr], [bg], fr, bg
        else:
            frc, bgc = cs.bgr()
            seg.set_background_color(bgc)
            seg.segment_color_host(list(frc))
            gray_fr, gray_bg = oracle.bgr2gray(frc), oracle.bgr2gray(bgc)
            if enc == capi.ENC_RGB8:
                self.planes, self.bgs = [frc[..., c] for c in range(3)], [bgc[..., c] for c in range(3)]
            else:
                self.planes, self.bgs = [np.stack([oracle.convert_to_r3g3b2(f) for f in frc])], [np.zeros((cs.H, cs.W), np.uint8)]
        self.res = seg.fetch()
        self.names = {}
        p = oracle.make_params(cs.W, cs.H)
        for f, r in enumerate(self.res):
            ob, orr, _ = oracle.segment(gray_fr[f], gray_bg, p)
            assert r.runs.tobytes() == orr.tobytes() and np.array_equal(r.blobs["n_runs"], ob["n_runs"])
            for name, k in cs.classify(f, r.blobs).items():
                self.names[int(r.info["blob_begin"]) + k] = name
        assert sorted(self.names.values()) == list("abcdefgh")       # the scene drifted: a path of the kernels would go untested
        self.total = n = sum(len(r.blobs) for r in self.res)
        self.och = 3 if enc == capi.ENC_RGB8 else 1
        outline = torch.zeros((n, MP, 2), dtype=torch.float32, device="cuda"); segs = torch.zeros((n, MP // 2 + 1, 4), dtype=torch.float32, device="cuda")
        info = torch.zeros((n, 8), dtype=torch.int32, device="cuda"); mid = torch.zeros((n, 25, 4), dtype=torch.float32, device="cuda")
        self.d_minfo = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
        seg.posture_device(n, outline.data_ptr(), segs.data_ptr(), info.data_ptr(), max_points=MP)
        seg.midline_device(n, MP, info.data_ptr(), segs.data_ptr(), mid.data_ptr(), self.d_minfo.data_ptr())
        seg.synchronize()
        self.minfo = self.d_minfo.cpu().numpy().view(capi.MIDLINE_INFO_DTYPE).reshape(-1)
        with_midline = {self.names[i] for i in range(n) if self.minfo[i]["status"] == 0}
        assert {"a", "b"} <= with_midline, with_midline               # the posture crops below are not all empty (b: per-tap as rgb8)
        # caller-supplied Midline::transform matrices, as in test_crops_gpu.py: a rotation about a point inside the bounding box, which
        # lands within 8 pixels of the crop centre (short midline lengths: normalize_image shifts by 0.4 len, legacy by len / 2)
        rng = np.random.default_rng(4)
        self.tr = np.zeros((n, 6), np.float32)
        self.ln = rng.uniform(2, 10, n).astype(np.float32)
        for r in self.res:
            for k, b in enumerate(r.blobs):
                a = rng.uniform(0, 2 * np.pi); c_, s_ = np.cos(a), np.sin(a)
                fx = rng.uniform(0.2, 0.8) * (int(b["x1"]) - int(b["x0"]) + 1); fy = rng.uniform(0.2, 0.8) * (int(b["y1"]) - int(b["y0"]) + 1)
                self.tr[int(r.info["blob_begin"]) + k] = [c_, -s_, -fx * c_ + fy * s_ - 3.0, s_, c_, -fx * s_ - fy * c_ + 2.0]

    def blobs(self):
        """(pooled index, class name, frame index, blob, runs of the frame)"""
        for f, r in enumerate(self.res):
            for k, b in enumerate(r.blobs):
                bi = int(r.info["blob_begin"]) + k
                yield bi, self.names[bi], f, b, r.runs

    def launch(self, call, ow, oh):
        """run `call(d_crops_ptr)` on a sentinel-filled buffer of total + 1 crops -> uint8 [total][oh][ow][och]"""
        d = torch.full((self.total + 1, oh, ow, self.och), SENTINEL, dtype=torch.uint8, device="cuda")
        call(d.data_ptr())
        self.seg.synchronize()
        got = d.cpu().numpy()
        assert (got[self.total] == SENTINEL).all(), "the crop behind the last one was written"
        return got[:self.total]

    def want_none(self, f, b, runs, ow, oh, difference):
        return np.stack([oracle.crop_none(pl[f], bg, b, runs, out_w=ow, out_h=oh, difference=difference, invert=self.invert)
                         for pl, bg in zip(self.planes, self.bgs)], axis=-1)

    def want_warp(self, f, b, runs, ow, oh, difference, **kw):
        return np.stack([oracle.crop_normalized(pl[f], bg, b, runs, out_w=ow, out_h=oh, difference=difference, invert=self.invert,
                                                nearest=self.enc == capi.ENC_R3G3B2, **kw)[0] for pl, bg in zip(self.planes, self.bgs)], axis=-1)


@pytest.fixture(scope="module")
def scenes():
    """the scene segmented once per encoding: "gray", "inv" (inverted frames under image_invert), "rgb8", "r3g3b2" """
    _scenes = {}

    def get(key):
        if key not in _scenes:
            _scenes[key] = Scene({"gray": capi.ENC_GRAY, "inv": capi.ENC_GRAY, "rgb8": capi.ENC_RGB8, "r3g3b2": capi.ENC_R3G3B2}[key], invert=key == "inv")
        return _scenes[key]
    yield get
    for s in _scenes.values():
        s.seg.close()


def check(sc, got, want_of, tag):
    nonzero = set()
    for bi, name, f, b, runs in sc.blobs():
        want = want_of(bi, f, b, runs)
        if want is None:
            assert not got[bi].any(), (tag, name, "no midline: empty crop")
            continue
        assert np.array_equal(got[bi], want), (tag, name, int((got[bi] != want).sum()), int(got[bi].any()), int(want.any()))
        if want.any():
            nonzero.add(name)
    return nonzero


# un-normalised crops show the centre of the bounding box: non-empty for every blob, but for the 16 x 16 centre of the ring, which is its hole
CENTRE_IN_HOLE = {(16, 16): {"c"}}

# (encoding, out_w, out_h, difference)
NONE_CASES = [("gray", 16, 16, 0), ("gray", 96, 40, 1), ("gray", 40, 96, 2), ("gray", 256, 256, 1), ("gray", 320, 16, 0), ("gray", 16, 320, 2),
              ("gray", 80, 80, 0), ("inv", 320, 16, 2), ("rgb8", 96, 40, 0), ("rgb8", 96, 40, 1), ("r3g3b2", 96, 40, 0)]


@pytest.mark.parametrize("enc,ow,oh,difference", NONE_CASES)
def test_crops_none(scenes, enc, ow, oh, difference):
    sc = scenes(enc)
    got = sc.launch(lambda p: sc.seg.crops_device(p, sc.total, out_w=ow, out_h=oh, difference=difference), ow, oh)
    nz = check(sc, got, lambda bi, f, b, runs: sc.want_none(f, b, runs, ow, oh, difference), ("none", enc, ow, oh, difference))
    assert nz == set("abcdefgh") - CENTRE_IN_HOLE.get((ow, oh), set())


MOMENTS_CASES = [("gray", 16, 16, 1), ("gray", 96, 40, 2), ("gray", 40, 96, 0), ("gray", 256, 256, 0), ("gray", 320, 16, 2), ("gray", 16, 320, 1),
                 ("gray", 80, 80, 2), ("inv", 96, 40, 1), ("rgb8", 96, 40, 1), ("r3g3b2", 96, 40, 0)]


@pytest.mark.parametrize("enc,ow,oh,difference", MOMENTS_CASES)
def test_crops_moments(scenes, enc, ow, oh, difference):
    sc = scenes(enc)
    got = sc.launch(lambda p: sc.seg.crops_device(p, sc.total, out_w=ow, out_h=oh, normalization=1, difference=difference), ow, oh)
    nz = check(sc, got, lambda bi, f, b, runs: sc.want_warp(f, b, runs, ow, oh, difference), ("moments", enc, ow, oh, difference))
    assert nz == set("abcdefgh")            # f and h included: no empty crop for a blob beyond the LDS tables
    if enc == "gray" and (ow, oh) == (256, 256):
        # the hole of c stays black: inside the ring's crop there is a connected all-zero region of the hole's size that the border does not touch
        from scipy import ndimage
        ci = next(bi for bi, name, *_ in sc.blobs() if name == "c")
        lab, n = ndimage.label(got[ci][..., 0] == 0)
        at_border = set(lab[0]) | set(lab[-1]) | set(lab[:, 0]) | set(lab[:, -1])
        assert max((lab == k).sum() for k in range(1, n + 1) if k not in at_border) >= 0.9 * 51 * 61


# (encoding, out_w, out_h, difference, legacy, scale)
TRANSFORMED_CASES = [("gray", 16, 16, 0, False, 1.0), ("gray", 96, 40, 1, True, 1.0), ("gray", 40, 96, 2, False, 1.0), ("gray", 256, 256, 2, True, 1.0),
                     ("gray", 320, 16, 1, False, 1.0), ("gray", 16, 320, 0, True, 1.0), ("gray", 80, 80, 1, False, 1.0), ("gray", 50, 50, 0, True, 1.0),
                     ("gray", 50, 50, 2, False, 1.7), ("gray", 96, 40, 0, False, 0.5), ("gray", 40, 96, 1, True, 1.7), ("inv", 40, 96, 2, False, 1.7),
                     ("rgb8", 96, 40, 2, False, 0.5), ("rgb8", 96, 40, 0, True, 1.7), ("r3g3b2", 96, 40, 0, False, 1.7)]


@pytest.mark.parametrize("enc,ow,oh,difference,legacy,scale", TRANSFORMED_CASES)
def test_crops_transformed(scenes, enc, ow, oh, difference, legacy, scale):
    sc = scenes(enc)
    got = sc.launch(lambda p: sc.seg.crops_transformed_device(p, sc.tr, sc.ln, out_w=ow, out_h=oh, legacy=legacy, scale=scale, difference=difference), ow, oh)
    nz = check(sc, got, lambda bi, f, b, runs: sc.want_warp(f, b, runs, ow, oh, difference, tr6=sc.tr[bi], midline_length=float(sc.ln[bi]), legacy=legacy, scale=scale),
               ("transformed", enc, ow, oh, difference, legacy, scale))
    if min(ow, oh) >= 40:
        assert {"b", "c", "f", "h"} <= nz   # both over-limit blobs and both per-tap blobs show something under these transforms


# (encoding, out_w, out_h, difference, legacy, scale, caller's lengths)
POSTURE_CASES = [("gray", 16, 16, 2, False, 1.0, False), ("gray", 96, 40, 0, False, 1.0, True), ("gray", 40, 96, 1, True, 1.0, False), ("gray", 256, 256, 1, False, 1.0, True),
                 ("gray", 320, 16, 2, True, 1.0, False), ("gray", 16, 320, 0, False, 1.0, True), ("gray", 80, 80, 0, False, 1.0, False), ("gray", 50, 50, 1, False, 1.0, True),
                 ("gray", 96, 40, 2, False, 0.5, False), ("gray", 40, 96, 0, True, 1.7, True), ("inv", 96, 40, 1, False, 1.0, True),
                 ("rgb8", 96, 40, 0, False, 1.7, True), ("rgb8", 96, 40, 1, False, 0.5, False), ("r3g3b2", 40, 96, 0, False, 1.0, True)]


@pytest.mark.parametrize("enc,ow,oh,difference,legacy,scale,own_lengths", POSTURE_CASES)
def test_crops_posture(scenes, enc, ow, oh, difference, legacy, scale, own_lengths):
    # posture -> midline -> k_warp_maps -> warp on the device; the oracle gets the device's Midline::angle() / offset() / len()
    sc = scenes(enc)
    mi = sc.minfo
    lengths = None
    if own_lengths:                                     # the individuals' median midline lengths: every one differs from the blob's own len()
        lengths = np.where(mi["status"] == 0, mi["len"] * 1.25 + 2.0 + np.arange(sc.total), 30.0).astype(np.float32)
        assert (np.abs(lengths - mi["len"]) > 1.0)[mi["status"] == 0].all()
    got = sc.launch(lambda p: sc.seg.crops_posture_device(p, sc.total, sc.d_minfo.data_ptr(), midline_lengths=lengths, out_w=ow, out_h=oh, legacy=legacy,
                                                          scale=scale, difference=difference), ow, oh)

    def want(bi, f, b, runs):
        if mi[bi]["status"] != 0:
            return None
        tr = oracle.midline_transform(mi[bi]["angle"], mi[bi]["offx"], mi[bi]["offy"], legacy)
        ln = float(lengths[bi]) if own_lengths else float(mi[bi]["len"])
        return sc.want_warp(f, b, runs, ow, oh, difference, tr6=tr, midline_length=ln, legacy=legacy, scale=scale)
    nz = check(sc, got, want, ("posture", enc, ow, oh, difference, legacy, scale, own_lengths))
    assert len(nz) >= 2
    if own_lengths:                                     # ... and the lengths matter: the blob's own len() gives another crop
        other = [bi for bi, name, f, b, runs in sc.blobs() if mi[bi]["status"] == 0 and not np.array_equal(
            got[bi], sc.want_warp(f, b, runs, ow, oh, difference, tr6=oracle.midline_transform(mi[bi]["angle"], mi[bi]["offx"], mi[bi]["offy"], legacy),
                                  midline_length=float(mi[bi]["len"]), legacy=legacy, scale=scale))]
        assert other


def test_untransformed_crops_refuse_sizes_that_are_no_multiple_of_16_bytes(scenes):
    # k_crops_none clears its crop with 16-byte stores; the warp writes single bytes (50 x 50 runs above)
    sc = scenes("gray")
    d = torch.full((sc.total + 1, 50, 50), SENTINEL, dtype=torch.uint8, device="cuda")
    for normalization in (0, 1):
        with pytest.raises(capi.TrexHipError) as e:
            sc.seg.crops_device(d.data_ptr(), sc.total, out_w=50, out_h=50, normalization=normalization)
        assert e.value.code == E_INVALID
    sc.seg.synchronize()
    assert (d.cpu().numpy() == SENTINEL).all()
