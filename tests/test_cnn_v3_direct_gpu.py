"""The listed conv3 reads the background rows of V3 from the empty crop's image itself (trex_amd/csrc/cnn_skip3.h: skip3_row_sources) and
k_v3_fill copies them only where the dense conv3 runs.  Every result must be, bit for bit, that of the chain that keeps the copy
(TREXHIP_CONV_GEOM bit 25), of the dense conv3 (bit 26) and of the two-kernel chain (bit 28).  A V3 row outside a crop's own rows is written by
nobody then and holds what an earlier call left there: the stale-row tests put noise there first.  Bit 29 forces the role-split chain at small
batches."""
import os
import numpy as np
import pytest
from trex_amd import weights
from cnn_skip_driver import blob, same, state  # noqa: F401  (state: the module's fixture)
import cnn_skip_driver

pytestmark = pytest.mark.gpu

RS, COPY, DENSE3, TWO = 1 << 29, 1 << 29 | 1 << 25, 1 << 29 | 1 << 26, 1 << 28
V3_ROWB = 10240


def forward(monkeypatch, st, geom, crops, **kw):
    """-> (probabilities, logits) of every call, skip_stats and skip3_stats of the last call"""
    outs, guard, stats = cnn_skip_driver.forward(monkeypatch, st, geom, crops, **kw)
    assert guard == (0, False)                               # background activations in range: nothing is re-run
    return outs, stats[-1].skip, stats[-1].skip3


def check(monkeypatch, st, crops):
    """the default chain against bit 25, bit 26 and bit 28 -> skip_stats, skip3_stats of the default chain"""
    on, s_on, s3_on = forward(monkeypatch, st, RS, crops)
    cp, s_cp, s3_cp = forward(monkeypatch, st, COPY, crops)
    off, s_off, _ = forward(monkeypatch, st, DENSE3, crops)
    two, _, _ = forward(monkeypatch, st, TWO, crops)
    assert np.all(np.isfinite(on[0][0])) and np.allclose(on[0][0].sum(1), 1.0, atol=1e-5)
    assert same(on[0], off[0]), float(np.abs(on[0][1] - off[0][1]).max())
    assert same(cp[0], off[0]), float(np.abs(cp[0][1] - off[0][1]).max())
    assert same(on[0], two[0]), float(np.abs(on[0][1] - two[0][1]).max())
    print("%d crops: skip %s, skip3 %s" % (len(crops), s_on, s3_on))
    assert s_on == s_cp == s_off and s3_on == s3_cp          # the counters do not know who supplies the rows
    return s_on, s3_on


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 80, 80, 1)).astype(np.uint8)


def test_one_empty_crop(monkeypatch, state):
    """nothing is listed: no pass of conv3 runs, all 20 rows count as taken from the image"""
    skip, skip3 = check(monkeypatch, state, np.zeros((1, 80, 80, 1), np.uint8))
    assert skip == (7, 0, 20 * V3_ROWB) and skip3[:3] == (10, 0, 0)


def test_one_pixel_in_row_r_of_crop_r(monkeypatch, state):
    """own rows of every position and length at both crop edges; most staged rows are image rows"""
    crops = np.zeros((80, 80, 80, 1), np.uint8)
    for r in range(80):
        crops[r, r, (37 * r + 11) % 80, 0] = 255
    skip, skip3 = check(monkeypatch, state, crops)
    assert skip3[2] > 0 and skip[2] > 0


def test_seven_crops_passes_straddle(monkeypatch, state):
    rng = np.random.default_rng(12)
    crops = np.zeros((7, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(0, 9), slice(20, 60), rng)           # touches row 0
    blob(crops, 1, slice(70, 80), slice(5, 75), rng)          # touches row 79
    blob(crops, 2, slice(0, 3), slice(0, 80), rng)
    crops[3, :, :, 0] = rng.integers(0, 256, (80, 80))        # full of noise
    blob(crops, 5, slice(33, 47), slice(30, 50), rng)         # crop 4 stays empty
    blob(crops, 6, slice(76, 80), slice(0, 10), rng)          # the last, partial pass
    skip, skip3 = check(monkeypatch, state, crops)
    assert skip3[2] == 5


def test_320_crops(monkeypatch, state):
    crops = weights.synthetic_crops(320, 4321).copy()
    crops[17] = 0
    crops[200] = noise(1, 1)[0]
    skip, skip3 = check(monkeypatch, state, crops)
    assert skip3[2] > 0 and 0 < skip[1] < skip[0]


def test_noise_runs_the_dense_form_and_the_fill_has_nothing_to_copy(monkeypatch, state):
    skip, skip3 = check(monkeypatch, state, noise(64, 8))
    assert skip3[:3] == (640, 640, 0) and skip[1] == skip[0] and skip[2] == 0


def test_conv2_skips_but_conv3_stays_dense(monkeypatch, state):
    """62 noise crops and two with one pixel: conv2 skips the passes of their background rows, conv3's listed passes (100 of noise, 4 and 2 pairs
    in two more) are more than the dense form's 100 -- the dense form needs whole rows, so the fill copies"""
    crops = noise(64, 9)
    crops[20] = 0; crops[20, 40, 17, 0] = 200
    crops[41] = 0; crops[41, 0, 3, 0] = 99
    skip, skip3 = check(monkeypatch, state, crops)
    assert skip3[2] == 0 and skip3[1] == 620 + 4 + 2 and skip[2] > 0 and skip[1] < skip[0]


def sparse(n, seed):
    crops = np.zeros((n, 80, 80, 1), np.uint8)
    src = weights.synthetic_crops(n, seed)
    for i in range(n):                                        # a band of 6 to 20 rows of every blob, somewhere else in every crop
        y0 = (7 * i) % 60
        crops[i, y0:y0 + 6 + i % 15] = src[i, y0:y0 + 6 + i % 15]
    crops[3] = 0
    return crops


@pytest.mark.parametrize("n", [24, 320])
def test_stale_rows_are_never_read(monkeypatch, state, n):
    """noise crops five times in the same device buffers -- every V3 row computed, none equal to the image, and from the fourth call on the
    replayed graph --, then sparse crops written in place and one more call: equal to a fresh context's dense conv3 on the sparse crops.  A row
    read from V3 that should have come from the image holds noise-derived bits"""
    assert os.environ.get("TREXHIP_GRAPHS", "1") != "0"
    first, then = noise(n, 21), sparse(n, 22)
    on, skip, skip3 = forward(monkeypatch, state, RS, first, calls=5, then=then)
    ref, _, _ = forward(monkeypatch, state, DENSE3, then)
    ref_noise, _, _ = forward(monkeypatch, state, DENSE3, first)
    for rep in range(5):
        assert same(on[rep], ref_noise[0]), rep
    assert same(on[5], ref[0]), float(np.abs(on[5][1] - ref[0][1]).max())
    assert skip3[2] > 0 and skip[2] > 0                      # the listed form ran, on rows nobody copied
    assert not same(on[5], on[4])
