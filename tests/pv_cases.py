"""Stored V_6 frame bodies shared by tests/test_pv_read.py (CPU: trex_amd/csrc/pv_read.h through tests/cpp/test_pv_read.cpp) and
tests/test_load_frames_gpu.py (the device loader, which applies the same header's rules): valid bodies from the oracle, and the list of
malformed ones, each made by editing one valid two-blob body."""
import numpy as np
from oracle import oracle
from trex_amd import synth

W, H = 320, 96


def frame_tables(blob_lines, pixel_seed=0):
    """[[(x0, x1, y), ...] per blob] -> (blobs, runs, pixels) as oracle.pv_serialize_v6 takes them (counts and offsets only)"""
    rng = np.random.default_rng(pixel_seed)
    blobs = np.zeros(len(blob_lines), oracle.BLOB_DTYPE)
    runs, ro, po = [], 0, 0
    for b, lines in enumerate(blob_lines):
        n_px = sum(x1 - x0 + 1 for x0, x1, _ in lines)
        blobs[b]["run_begin"], blobs[b]["n_runs"], blobs[b]["pix_begin"], blobs[b]["n_pixels"] = ro, len(lines), po, n_px
        runs += [(x0, x1, y, 0) for x0, x1, y in lines]
        ro += len(lines); po += n_px
    return blobs, np.array(runs, oracle.RUN_DTYPE).reshape(-1), rng.integers(1, 256, po, dtype=np.uint8)


def scene(seed):
    fr, bg = synth.random_scene(np.random.default_rng(seed), W, H, density=0.12)
    return oracle.segment(fr, bg, oracle.make_params(W, H))


LITERAL = [[(10, 12, 7), (20, 21, 7), (9, 13, 8)]]                      # the three-line literal of tests/test_pv_frames.py (start_y 7)
TWO_BLOBS = [[(10, 12, 7), (20, 21, 7), (9, 13, 8)], [(300, 319, 94), (310, 319, 95)]]


def two_blob_body():
    return oracle.pv_serialize_v6(*frame_tables(TWO_BLOBS, 5), timestamp=77)


def _put16(a, at, v):
    a[at] = v & 0xff; a[at + 1] = v >> 8


def malformed_cases():
    """{name: body}: every entry is two_blob_body() with ONE edit (pixel bytes are added / removed with a line edit so that only the
    named rule is broken).  Offsets: frame head 11; blob A head at 11, its lines at 15, 19, 23, its 10 pixels at 27; blob B head at 37,
    its lines at 41, 45, its 30 pixels at 49; 79 bytes in all."""
    good = two_blob_body()
    assert len(good) == 79
    out = {}
    for k in range(len(good)):
        out["cut_%d" % k] = good[:k].copy()
    e = good.copy(); e[0] = 1
    out["flag_1"] = e
    e = good.copy(); _put16(e, 13, 0)
    out["mask_size_0"] = e
    e = good.copy(); _put16(e, 43, (W << 1) | 1)                             # blob B's first line (300, 319) -> x1 = width; one pixel more
    out["x1_is_width"] = np.concatenate([e, [9]]).astype(np.uint8)
    e = good.copy(); _put16(e, 19, 22)                                       # blob A's (20, 21) -> x0 = 22 > x1; its two pixels leave
    out["x0_above_x1"] = np.concatenate([e[:30], e[32:]]).astype(np.uint8)
    e = good.copy(); _put16(e, 37, 95)                                       # blob B starts on the last row: its second line is on row `height`
    out["y_is_height"] = e
    e = good.copy(); _put16(e, 19, 12)                                       # blob A's (20, 21) -> (12, 21): overlaps (10, 12) of the same row; 8 pixels more
    out["overlap_on_a_row"] = np.concatenate([e[:30], np.full(8, 3, np.uint8), e[30:]]).astype(np.uint8)
    out["trailing_byte"] = np.concatenate([good, [0]]).astype(np.uint8)
    return out


CUT_INSIDE_PIXELS = "cut_60"                                                # inside blob B's pixel bytes
