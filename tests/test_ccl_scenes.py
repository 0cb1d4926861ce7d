"""The conditions the shared labelling-path scenes (tests/ccl_scenes.py) have to meet, from the oracle's tables alone: a change of a generator
cannot quietly move a frame out of its line-count class, into overflow, or out of it.  The GPU tests assert the same before they run."""
import numpy as np
import pytest
import ccl_scenes as cs


def test_textured_ladder_keeps_its_brackets_and_fits():
    cs.check_ladder()
    bg, distinct = cs.textured_ladder()
    assert [len(cs.detect_tables(("ladder", k))[1]) for k in range(6)] == [742, 160, 2618, 2888, 4117, 5504]


def test_band_and_global_chain_scenes_fit():
    bg, frames = cs.textured_band_frames()
    keys = [cs.register(("band", i), bg, f) for i, f in enumerate(frames)]
    for conn in (8, 4):
        for k in keys[:-1]:
            cs.check_capacities(k, cs.BAND_CAPS, connectivity=conn)
            assert len(cs.detect_tables(k)[1]) <= cs.CCL_NMAX
    obg, of = cs.odd_height_frame()
    assert of.shape == (1000, 640)
    cs.check_capacities(cs.register("odd_height", obg, of), cs.BAND_CAPS)
    bg, frames = cs.global_chain_frames()
    keys = [cs.register(("chain", i), bg, f) for i, f in enumerate(frames)]
    for k in keys[:2]:
        cs.check_capacities(k, cs.BAND_CAPS)
    assert len(cs.detect_tables(keys[0])[1]) > cs.CCL_NMAX >= len(cs.detect_tables(keys[1])[1]) > 0 == len(cs.detect_tables(keys[2])[1])


def test_pass2_overflow_scenes():
    cs.check_pass2_overflow()
    cs.check_pass2_many_blobs()


@pytest.mark.parametrize("method", [0, 1])
def test_per_blob_scene(method):
    cs.check_per_blob_scene(method)


def test_settings_scene_drops_and_keeps():
    bg, fr = cs.settings_scene()
    key = cs.register(("settings", "size_filter"), bg, fr)
    n_all, n_kept = len(cs.detect_tables(key)[0]), len(cs.detect_tables(key, **cs.SETTINGS_CASES["size_filter"])[0])
    assert 0.3 * n_all < n_kept < 0.7 * n_all, (n_all, n_kept)


def test_wide_frames_cross_the_chunk_border():
    for W in (2050, 2080, 4096):
        bg, frames = cs.wide_frames(W, 3)
        for i, fr in enumerate(frames):
            runs = cs.detect_tables(cs.register(("wide", W, 3, i), bg, fr))[1]
            assert np.any((runs["x0"] <= 2047) & (runs["x1"] >= 2048)) and np.any(runs["x1"] == W - 1)
