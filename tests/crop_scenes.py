"""Frames for the crop tests: one blob per path of the crop kernels (crops.hip), shared by the CPU test that pins the blobs' properties
(test_crops_oracle.py) and the device tests (test_crops_sizes_gpu.py).  Everything is a fixed function of (x, y): no random state.

Three frames of W x H = 320 x 1100 over one textured background, gray and BGR with the same geometry:
  frame 0   a  small body, bounding box <= 5461 pixels: painted into LDS in every encoding (3 bytes per pixel included)
            b  about 90 x 90: painted into LDS as gray, per-tap line tests as rgb8
            c  150 x 180 ring with a 50 x 60 hole: per-tap line tests in every encoding, the hole has to stay black
            d  300 x 7 strip in the top left corner: cut on one axis, padded on the other at every output size
            e  bar of exactly 1024 rows: the most rows whose line table fits into LDS
  frame 1   f  bar of 1040 rows: beyond the row table
            g  comb of exactly 2048 lines: the most lines held in LDS
  frame 2   h  comb of 2794 lines: beyond the line table
Blob pixels are 10..80 or, for about a quarter of them, 180..250; the background is 104..136.  So the detect threshold of 15 keeps
exactly the painted masks (with image_invert as well), and |bg - p| differs from max(bg - p, 0) on the bright pixels."""
import numpy as np

W, H = 320, 1100
N_FRAMES = 3
W_IMG = 16384           # crops.hip: bounding boxes of up to this many bytes are painted into LDS
W_NR, W_ROWS = 2048, 1024   # crops.hip: lines / rows of one blob held in LDS

# name -> (frame, x0, y0, x1, y1): the bounding boxes that masks() paints (test_crops_oracle.py holds them to the segmentation)
BOXES = {"a": (0, 19, 43, 71, 77), "b": (0, 108, 28, 192, 112), "c": (0, 20, 160, 170, 340), "d": (0, 0, 0, 299, 6),
         "e": (0, 298, 30, 312, 1053), "f": (1, 290, 20, 301, 1059), "g": (1, 100, 10, 169, 524), "h": (2, 100, 10, 169, 709)}
# output sizes (out_w, out_h) of the device tests; 80 x 80 is the control, 50 x 50 no multiple of 16 bytes
SIZES = [(16, 16), (96, 40), (40, 96), (256, 256), (320, 16), (16, 320), (80, 80), (50, 50)]


def _hash(x, y, salt):
    h = (x.astype(np.uint32) * np.uint32(73856093)) ^ (y.astype(np.uint32) * np.uint32(19349663)) ^ np.uint32(salt * 83492791 + 12345)
    h ^= h >> np.uint32(13); h *= np.uint32(0x5bd1e995); h ^= h >> np.uint32(15)
    return h


def _ellipse(xx, yy, cx, cy, a, b, th):
    u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
    v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
    return (u / a) ** 2 + (v / b) ** 2 <= 1


def _comb(mask, ox, oy, tooth_rows, extra_rows_first_tooth=0):
    """teeth at ox + {0, 20, 40, 60}, 10 wide, below a two-row spine: 2 + 4 * tooth_rows (+ extra) lines"""
    mask[oy:oy + 2, ox:ox + 70] = True
    for k in range(4):
        rows = tooth_rows + (extra_rows_first_tooth if k == 0 else 0)
        mask[oy + 2:oy + 2 + rows, ox + 20 * k:ox + 20 * k + 10] = True


def masks():
    """bool [3][H][W]: the blobs' pixels"""
    m = np.zeros((N_FRAMES, H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    m[0] |= _ellipse(xx, yy, 45, 60, 30, 11, 0.5)                                         # a
    m[0] |= _ellipse(xx, yy, 150, 70, 52, 30, np.pi / 4)                                  # b
    m[0] |= _ellipse(xx, yy, 95, 250, 75, 90, 0.0) & ~((np.abs(xx - 80) <= 25) & (np.abs(yy - 230) <= 30))   # c
    m[0, 0:7, 0:300] = True                                                               # d
    for yi in range(30, 30 + 1024):                                                       # e: 10..14 wide, ragged edges
        m[0, yi, 298 + (yi * 7) % 3:310 + (yi * 5) % 4] = True
    for yi in range(20, 20 + 1040):                                                       # f: box 12 x 1040 (painted into LDS as gray)
        m[1, yi, 290 + (yi * 3) % 2:301 + (yi * 5) % 2] = True
    _comb(m[1], 100, 10, 511, extra_rows_first_tooth=2)                                   # g: 2 + 4 * 511 + 2 = 2048 lines, 515 rows
    _comb(m[2], 100, 10, 698)                                                             # h: 2 + 4 * 698 = 2794 lines, 700 rows
    return m


def gray():
    """-> frames uint8 [3][H][W], background uint8 [H][W]"""
    y, x = np.mgrid[0:H, 0:W]
    bg = (120 + ((x * 3 + y * 5) & 31) - 16).astype(np.uint8)
    h = _hash(x, y, 1)
    dark = 10 + (h >> np.uint32(8)) % np.uint32(71)
    bright = 180 + (h >> np.uint32(8)) % np.uint32(71)
    body = np.where((h & np.uint32(3)) == 0, bright, dark).astype(np.uint8)
    fr = np.where(masks(), body[None], bg[None]).astype(np.uint8)
    return fr, bg


def bgr():
    """-> frames uint8 [3][H][W][3], background uint8 [H][W][3]: the same masks; a pixel is dark or bright in all three channels"""
    y, x = np.mgrid[0:H, 0:W]
    bgc = np.stack([(120 + ((x * (3 + 2 * c) + y * (5 + 2 * c)) & 31) - 16) for c in range(3)], axis=-1).astype(np.uint8)
    sel = (_hash(x, y, 1) & np.uint32(3)) == 0
    body = np.zeros((H, W, 3), np.uint8)
    for c in range(3):
        v = (_hash(x, y, 2 + c) >> np.uint32(8)) % np.uint32(71)
        body[..., c] = np.where(sel, 180 + v, 10 + v)
    fr = np.where(masks()[..., None], body[None], bgc[None]).astype(np.uint8)
    return fr, bgc


def classify(f, blobs):
    """{class name: index} of the blobs of frame f whose bounding box is one of BOXES"""
    out = {}
    for k, b in enumerate(blobs):
        box = (f, int(b["x0"]), int(b["y0"]), int(b["x1"]), int(b["y1"]))
        for name, want in BOXES.items():
            if box == want:
                out[name] = k
    return out
