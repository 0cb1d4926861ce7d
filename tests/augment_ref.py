"""The yardstick of the device augmentation (trexhip_augment_device): the reference's training transform -- torchvision
RandomAffine(degrees, translate) then ColorJitter(brightness, contrast, saturation, hue) inside TRexImageDataset.__getitem__
(visual_recognition_torch.py:158-194, :1325-1331) -- restated twice for GIVEN draws, over a batch:

  (a) augment64: the formulas in numpy float64 (what the device is held to);
  (b) augment32: torch CPU float32, operation for operation what torchvision runs on a float tensor: the inverse matrix in Python
      floats, affine_grid-style linspace / bmm, grid_sample(nearest, zeros, align_corners=False), then the tensor forms of
      adjust_brightness / contrast / saturation / hue (_blend, rgb_to_grayscale, _rgb2hsv, _hsv2rgb).

E32 = max |(b) - (a)| is the fp32 restatement's own error; the device gets 8 x E32 (tests/test_augment_gpu.py).  torchvision itself is not
installed, so nothing here imports it.  Images are uint8 [n][H][W][C]; a draw is one record of DRAW_DTYPE (= trexhip_augment_draw);
results are [n][H][W][C] in [0, 255]."""
import itertools
import math

import numpy as np
import torch

DRAW_DTYPE = np.dtype([("angle", "<f4"), ("tx", "<i4"), ("ty", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                       ("hue", "<f4"), ("order", "<i4")])
IDENTITY_ORDER = 0xE4            # brightness, contrast, saturation, hue: 2 bits each, first operation lowest
BAND = 1e-3                      # px: a source coordinate this close to a half-integer is a near-tie of the nearest-neighbour choice


def make_draws(n, angle=0.0, tx=0, ty=0, brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, order=IDENTITY_ORDER):
    d = np.zeros(n, DRAW_DTYPE)
    for k, v in dict(angle=angle, tx=tx, ty=ty, brightness=brightness, contrast=contrast, saturation=saturation, hue=hue, order=order).items():
        d[k] = v
    return d


def pack_order(perm):
    return sum(int(op) << (2 * k) for k, op in enumerate(perm))


def unpack_order(order):
    return [(int(order) >> (2 * k)) & 3 for k in range(4)]


# ---- (a) float64 ------------------------------------------------------------------------------------------------------------------

def source_coords(d, W, H):
    """unrounded source column / row of every output pixel, float64 [n][H][W] each"""
    rad = np.deg2rad(d["angle"].astype(np.float64))[:, None, None]
    c, s = np.cos(rad), np.sin(rad)
    tx, ty = d["tx"].astype(np.float64)[:, None, None], d["ty"].astype(np.float64)[:, None, None]
    xo = (np.arange(W) - W / 2 + 0.5)[None, None, :]
    yo = (np.arange(H) - H / 2 + 0.5)[None, :, None]
    return c * xo + s * yo - c * tx - s * ty + W / 2 - 0.5, -s * xo + c * yo + s * tx - c * ty + H / 2 - 0.5


def band(d, W, H):
    """bool [n][H][W]: the pixels whose source column or row lies within BAND of a half-integer"""
    fx, fy = source_coords(d, W, H)
    return (np.abs(fx - np.floor(fx) - 0.5) <= BAND) | (np.abs(fy - np.floor(fy) - 0.5) <= BAND)


def affine64(images, d):
    n, H, W, _ = images.shape
    fx, fy = source_coords(d, W, H)
    sx, sy = np.rint(fx), np.rint(fy)                                       # half to even
    inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
    sxi, syi = np.clip(sx, 0, W - 1).astype(np.int64), np.clip(sy, 0, H - 1).astype(np.int64)
    return images[np.arange(n)[:, None, None], syi, sxi].astype(np.float64) * inside[..., None]


def _gray64(x):
    return 0.2989 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]


def _hue64(x, f):
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(axis=-1), x.min(axis=-1)
    eq = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eq, 1.0, maxc)
    div = np.where(eq, 1.0, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = (maxc == r) * (bc - gc) + ((maxc == g) & (maxc != r)) * (2.0 + rc - bc) + ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = np.fmod(h / 6.0 + 1.0, 1.0)
    h = np.mod(h + f, 1.0)
    v = maxc
    i = np.floor(h * 6.0)
    ff = h * 6.0 - i
    i = i.astype(np.int64) % 6
    p = np.clip(v * (1.0 - s), 0, 1)
    q = np.clip(v * (1.0 - s * ff), 0, 1)
    t = np.clip(v * (1.0 - s * (1.0 - ff)), 0, 1)
    table = np.stack([np.stack(c, -1) for c in ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))], 0)      # [6][...][3]
    return np.take_along_axis(table, i[None, ..., None], 0)[0]


def jitter64(x, d):
    """x float64 [n][H][W][C] in [0, 1] -> the same after the draws' four operations, each in its sample's order"""
    x = x.copy()
    C = x.shape[-1]
    for k in range(4):
        op = (d["order"].astype(np.int64) >> (2 * k)) & 3
        for o in range(4):
            sel = np.nonzero(op == o)[0]
            if not len(sel) or (C == 1 and o >= 2):
                continue
            y = x[sel]
            if o == 0:
                y = y * d["brightness"][sel].astype(np.float64)[:, None, None, None]
            elif o == 1:
                f = d["contrast"][sel].astype(np.float64)[:, None, None, None]
                m = (_gray64(y) if C == 3 else y[..., 0]).mean(axis=(1, 2))[:, None, None, None]
                y = f * y + (1.0 - f) * m
            elif o == 2:
                f = d["saturation"][sel].astype(np.float64)[:, None, None, None]
                y = f * y + (1.0 - f) * _gray64(y)[..., None]
            else:
                y = _hue64(y, d["hue"][sel].astype(np.float64)[:, None, None])
            x[sel] = np.clip(y, 0.0, 1.0)
    return x


def augment64(images, d):
    return np.clip(jitter64(affine64(images, d) / 255.0, d), 0.0, 1.0) * 255.0


def plain(images):
    """the validation loader (transform=None)"""
    return images.astype(np.float32)


# ---- (b) torch float32, as torchvision does it ---------------------------------------------------------------------------------------

def _inverse_matrix(angle, tx, ty):
    # torchvision's _get_inverse_affine_matrix(center=(0, 0), angle, translate, scale=1, shear=(0, 0)), in Python floats
    rot = math.radians(angle)
    a, b, c, dd = math.cos(rot), -math.sin(rot), math.sin(rot), math.cos(rot)
    m = [dd, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-tx) + m[1] * (-ty)
    m[5] += m[3] * (-tx) + m[4] * (-ty)
    return m


def affine32(x, d):
    """x float32 tensor [n][C][H][W] -> F.affine(nearest, fill 0) of every sample with its draw"""
    n, _, H, W = x.shape
    theta = torch.tensor([_inverse_matrix(float(r["angle"]), float(r["tx"]), float(r["ty"])) for r in d], dtype=torch.float32).reshape(n, 2, 3)
    base = torch.empty(n, H, W, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + 0.5, W * 0.5 + 0.5 - 1, steps=W))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + 0.5, H * 0.5 + 0.5 - 1, steps=H).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32)
    grid = base.view(n, H * W, 3).bmm(rescaled).view(n, H, W, 2)
    return torch.nn.functional.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False)


def _gray32(x):
    r, g, b = x.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3)


def _blend32(a, b, ratio):
    return (ratio * a + (1.0 - ratio) * b).clamp(0, 1)


def _hue32(img, f):
    r, g, b = img.unbind(dim=-3)
    maxc, minc = torch.max(img, dim=-3).values, torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / cr_divisor, (maxc - g) / cr_divisor, (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + f) % 1.0
    v = maxc
    i = torch.floor(h * 6.0)
    ff = h * 6.0 - i
    i = i.to(torch.int32)
    p = torch.clamp(v * (1.0 - s), 0.0, 1.0)
    q = torch.clamp(v * (1.0 - s * ff), 0.0, 1.0)
    t = torch.clamp(v * (1.0 - (s * (1.0 - ff))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6).view(-1, 1, 1)
    a4 = torch.stack((torch.stack((v, q, p, p, t, v), dim=-3), torch.stack((t, v, v, q, p, p), dim=-3), torch.stack((p, p, t, v, v, q), dim=-3)), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def jitter32(x, d):
    x = x.clone()
    C = x.shape[1]
    for k in range(4):
        op = (d["order"].astype(np.int64) >> (2 * k)) & 3
        for o in range(4):
            sel = np.nonzero(op == o)[0]
            if not len(sel) or (C == 1 and o >= 2):
                continue
            y = x[sel]
            col = lambda name: torch.from_numpy(d[name][sel].astype(np.float32)).view(-1, 1, 1, 1)
            if o == 0:
                y = _blend32(y, torch.zeros_like(y), col("brightness"))
            elif o == 1:
                m = torch.mean(_gray32(y) if C == 3 else y, dim=(-3, -2, -1), keepdim=True)
                y = _blend32(y, m, col("contrast"))
            elif o == 2:
                y = _blend32(y, _gray32(y), col("saturation"))
            else:
                y = _hue32(y, col("hue")[:, 0])
            x[sel] = y
    return x


def augment32(images, d):
    x = torch.from_numpy(images).to(torch.float32).permute(0, 3, 1, 2).contiguous().div(255.0)
    x = jitter32(affine32(x, d), d)
    return (x.clamp(0.0, 1.0) * 255.0).permute(0, 2, 3, 1).contiguous().numpy()


# ---- inputs the tests share ----------------------------------------------------------------------------------------------------------

def sample_images(n, H, W, C, seed=0):
    """random bytes with the special images in front (as far as n goes): all 0, all 255, constant gray, and for three channels pure and
    mixed primaries (every hue sector and its edges) and a near-gray image"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n, H, W, C), dtype=np.uint8)
    special = [np.zeros((H, W, C), np.uint8), np.full((H, W, C), 255, np.uint8), np.full((H, W, C), 97, np.uint8)]
    if C == 3:
        prim = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [255, 128, 0], [128, 255, 0], [0, 255, 128],
                         [0, 128, 255], [128, 0, 255], [255, 0, 128], [200, 200, 100], [100, 200, 200], [200, 100, 200], [1, 0, 0], [254, 255, 255]], np.uint8)
        special.append(prim[np.arange(H * W) % len(prim)].reshape(H, W, 3))
        special.append((rng.integers(0, 2, (H, W, 3)) + 120).astype(np.uint8))
    for i, s in enumerate(special[:max(n - 1, 0)]):            # at least one random image stays
        x[i] = s
    return x


def value_draw_kinds():
    """the jitter settings of the value cases: all 24 orders with every factor at one end and at the other, then each factor alone at both
    ends and at its neutral value -- 60 kinds"""
    kinds = []
    for perm in itertools.permutations(range(4)):
        kinds.append(dict(order=pack_order(perm), brightness=1.15, contrast=0.85, saturation=1.15, hue=0.05))
        kinds.append(dict(order=pack_order(perm), brightness=0.85, contrast=1.15, saturation=0.85, hue=-0.05))
    for k, lo, hi in (("brightness", 0.85, 1.15), ("contrast", 0.85, 1.15), ("saturation", 0.85, 1.15), ("hue", -0.05, 0.05)):
        for v in (lo, hi, 0.0 if k == "hue" else 1.0):
            kinds.append({k: v})
    return kinds


def value_cases(C, H, W, per_kind=9, kinds=None):
    """(images, draws): angle 0 with whole shifts (exact geometry, no band), every kind of value_draw_kinds() on `per_kind` of the nine
    sample images (which ones rotates with the kind)"""
    kinds = value_draw_kinds() if kinds is None else kinds
    shifts = [(0, 0), (1, -2), (-1, 1)]
    pool = sample_images(9, H, W, C, seed=3)
    imgs, draws = [], []
    for i, kw in enumerate(kinds):
        pick = (np.arange(per_kind) + i * per_kind) % len(pool)
        imgs.append(pool[pick])
        draws.append(make_draws(per_kind, tx=shifts[i % 3][0], ty=shifts[i % 3][1], **kw))
    return np.concatenate(imgs), np.concatenate(draws)


def random_draws(n, W, H, seed, translate=None, jitter=True, empty_band=False):
    """what RandomAffine(5, translate).get_params and ColorJitter(0.85..1.15, +-0.05).get_params draw, from numpy's generator; translate None =
    the reference's move_range.  empty_band: affine draws are redrawn until no pixel of the sample lies in the near-tie band"""
    rng = np.random.default_rng(seed)
    t = min(0.05, 2 / min(W, H)) if translate is None else translate
    d = make_draws(n)
    for i in range(n):
        while True:
            d[i:i + 1]["angle"], d[i:i + 1]["tx"], d[i:i + 1]["ty"] = rng.uniform(-5, 5), np.rint(rng.uniform(-t * W, t * W)), np.rint(rng.uniform(-t * H, t * H))
            if not empty_band or not band(d[i:i + 1], W, H).any():
                break
    if jitter:
        for k in ("brightness", "contrast", "saturation"):
            d[k] = rng.uniform(0.85, 1.15, n)
        d["hue"] = rng.uniform(-0.05, 0.05, n)
        d["order"] = [pack_order(rng.permutation(4)) for _ in range(n)]
    return d
