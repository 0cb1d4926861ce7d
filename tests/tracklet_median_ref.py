"""The median image of a tracklet's crops as the reference computes it, restated line by line:
  hist_utils::Hist / init / addImage   Application/src/tracker/ui/Export.cpp:78-154
  the loop over a tracklet's images    Export.cpp:1287-1364 (gray conversion :1320-1327, the `image_count > 1` rule :1355)
NumPy does every pixel of an image at once; per pixel the operations and their order are the reference's."""
import numpy as np

MAX_ROWS = 32767          # Hist::h is vector<short> (:85-89): one more image in a bin overflows it


def bgr2gray(img):
    """cv::cvtColor(mat, tmp, cv::COLOR_BGR2GRAY) on uint8 [..., 3] in B, G, R memory order (:1326): OpenCV's 8-bit fixed point"""
    c = np.asarray(img, np.uint8).astype(np.uint32)
    return ((c[..., 0] * 1868 + c[..., 1] * 9617 + c[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def to_gray(img):
    """:1320-1328: one channel is copied, three go through BGR2GRAY, anything else throws"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    if img.shape[-1] == 1:
        return img[..., 0].copy()
    if img.shape[-1] == 3:
        return bgr2gray(img)
    raise ValueError(f"Invalid number of channels: {img.shape[-1]}")


def init(rows, cols):
    """hist_utils::init (:145-153): med = Mat1b(rows, cols, uchar(0)), every pixel a Hist{h(256, 0), count = 0}"""
    return {"h": np.zeros((rows, cols, 256), np.int16), "count": np.zeros((rows, cols), np.int32), "med": np.zeros((rows, cols), np.uint8)}


def walk(h, count):
    """:105-110 for every pixel: n = count / 2; for (i = 0; i < 256 && ((n -= h[i]) >= 0); ++i); -> uchar(i)"""
    n = (count // 2).astype(np.int32)
    i = np.zeros(count.shape, np.uint32)
    running = np.ones(count.shape, bool)
    for k in range(256):
        # the condition is evaluated for i = k where the loop still runs: n -= h[k], stop unless n >= 0
        n = np.where(running, n - h[..., k].astype(np.int32), n)
        running &= n >= 0
        i = np.where(running, k + 1, i)
    return i.astype(np.uint8)                                           # uchar(256) = 0: reached only by a pixel without samples


def add_image(state, gray):
    """hist_utils::addImage (:91-116)"""
    gray = np.asarray(gray, np.uint8)
    assert gray.shape == state["med"].shape
    r, c = np.indices(gray.shape)
    assert (state["h"][r, c, gray] < MAX_ROWS).all(), "a short bin would overflow: undefined in the reference"
    state["h"][r, c, gray] += np.int16(1)                               # ++hist.h[img(r, c)]
    state["count"] += 1                                                 # ++hist.count
    state["med"] = walk(state["h"], state["count"])
    return state["med"]


def final_median(hist, count):
    """the same walk applied once to finished histograms [..., 256] and counts [...]: what survives the last addImage"""
    hist = np.asarray(hist)
    count = np.asarray(count)
    if (count == 0).all():
        return np.zeros(count.shape, np.uint8)                          # the image init leaves: addImage never ran
    return np.where(count > 0, walk(hist.astype(np.int16), count.astype(np.int32)), 0).astype(np.uint8)


def histograms(stack):
    """uint8 [m][...] -> int32 counts [...][256]"""
    stack = np.asarray(stack, np.uint8)
    out = np.zeros(stack.shape[1:] + (256,), np.int32)
    flat = out.reshape(-1, 256)
    px = stack.reshape(len(stack), -1)
    for j in range(px.shape[1]):
        flat[j] = np.bincount(px[:, j], minlength=256)
    return out


def tracklet_median(images):
    """the loop of :1292-1348 for one tracklet: init, then addImage per (gray of an) image -> (med, image_count)"""
    images = list(images)
    assert images, "use init() for a tracklet without images"
    first = to_gray(images[0])
    st = init(*first.shape)
    for im in images:
        add_image(st, to_gray(im))
    return st["med"], len(images)


def medians(crops, tracklet, n_tracklets, incremental=True):
    """what trexhip_tracklet_medians_device is held to: crops uint8 [n][H][W][C], tracklet int [n] (-1 = none) ->
    (uint8 [T][H][W], uint32 [T]).  incremental=False takes final_median on the finished histograms (for counts where the walk per image
    is too slow; tests/test_tracklet_median_ref.py shows the two are equal)."""
    crops = np.asarray(crops, np.uint8)
    tracklet = np.asarray(tracklet)
    n, H, W = crops.shape[:3]
    med = np.zeros((n_tracklets, H, W), np.uint8)
    rows = np.zeros(n_tracklets, np.uint32)
    for t in range(n_tracklets):
        mine = np.flatnonzero(tracklet == t)
        rows[t] = len(mine)
        if len(mine) == 0:
            continue
        if incremental:
            med[t] = tracklet_median(crops[i] for i in mine)[0]
        else:
            g = np.stack([to_gray(crops[i]) for i in mine])
            med[t] = final_median(histograms(g), np.full((H, W), len(mine), np.int32))
    return med, rows
