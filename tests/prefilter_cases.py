"""Hand-worked scenes for the prefilter tests: 64 x 48 frames on a flat background of 200, blobs painted as rectangles of one grey value
(difference = 200 - value), so that every pixel count can be checked on paper.  Detect threshold 15 (absolute difference)."""
import numpy as np

W, H, BG = 64, 48, 200


def background():
    return np.full((H, W), BG, np.uint8)


def paint(rects):
    """rects: (x0, y0, x1, y1, value), inclusive corners, later ones paint over earlier ones."""
    f = background()
    for x0, y0, x1, y1, v in rects:
        f[y0:y1 + 1, x0:x1 + 1] = v
    return f


def blob_at(table, x, y):
    """Index of the blob of a frame table whose lines cover pixel (x, y)."""
    for k, b in enumerate(table.blobs):
        for r in table.runs[int(b["run_begin"]):int(b["run_begin"]) + int(b["n_runs"])]:
            if int(r["y"]) == y and int(r["x0"]) <= x <= int(r["x1"]):
                return k
    raise KeyError((x, y))


# --- scenes.  Differences: 100 = strong (value 100), 40 = medium (160), 20 = weak (180: passes detect 15, fails track 30) ---------------
SIZES = [(4, 4, 9, 8, 100),          # 6 x 5 = 30 px: inside (20, 100)
         (20, 4, 21, 5, 100),        # 2 x 2 = 4 px: below; 4 < 20 * 0.5 keeps the gate shut
         (30, 4, 41, 13, 100)]       # 12 x 10 = 120 px: above -> big
DUMBBELL = [(4, 20, 9, 24, 100),     # 30 px lobe
            (10, 22, 13, 22, 180),   # weak bridge: gone at track_threshold 30
            (14, 21, 16, 22, 100)]   # 3 x 2 = 6 px lobe
WEAK = [(30, 30, 34, 34, 180)]       # 25 px, nothing survives track_threshold 30
SECOND_IN = [(4, 30, 9, 34, 160), (4, 30, 8, 32, 100)]      # 30 px at 30, 5 x 3 = 15 px at 60: 15 >= 0.5 * 30
SECOND_OUT = [(20, 30, 25, 34, 160), (20, 30, 23, 32, 100)]   # 30 px at 30, 4 x 3 = 12 px at 60: 12 < 0.5 * 30
SHAPE_BLOBS = [(10, 10, 13, 13, 100),    # centre (12, 12)
               (10, 30, 13, 32, 100),    # 4 x 3, centre (12, 31.5)
               (2, 40, 5, 43, 100)]      # centre (4, 42)
L_SHAPE = [(0, 0), (30, 0), (30, 30), (20, 30), (20, 12), (0, 12)]     # concave: the notch is x < 20, y > 12

# run-length edges for the second count: a 1-pixel line, a line of 41 pixels that starts unaligned and crosses 16-byte boundaries, and a
# line that ends at the frame's last column; medium pixels everywhere, strong ones scattered
def run_edge_frame():
    f = background()
    f[5, 7:48] = 160
    f[5, 9:44:3] = 100
    f[6, 7] = 100                        # 1-pixel line under the long one's first pixel
    f[20, 30:64] = 160                   # ends at column 63
    f[20, 61:64] = 100
    f[21, 40:64] = 160
    f[21, 63] = 100
    return f
