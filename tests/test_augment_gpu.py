"""trexhip_augment_device on the GPU against the float64 formulas of tests/augment_ref.py (a).

The bar is 8 x E32, the multiple this project grants a device path over its fp32 restatement's own error against float64
(tests/test_cnn_trained_gpu.py): E32 = max |(b) - (a)| with (b) the torch-CPU-float32 restatement of what torchvision runs, taken in the
same test on the same inputs (never from the device's output).  Where rotation makes the nearest-neighbour choice a near-tie -- a float64
source coordinate within 1e-3 px of a half-integer, the "band" -- the pixel is left out, for E32 and for the device alike; the band may
hold at most 1 % of a case's pixels."""
import numpy as np
import pytest
import torch

import augment_ref as ref
from trex_amd import capi, train_loop

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 1), (9, 11, 3), (80, 80, 1), (80, 80, 3), (256, 256, 3)]        # (W, H, C); 256 x 256 x 3 is past the LDS staging
ANGLES = [0.0, 5.0, -5.0, 2.37, -2.37, 90.0, 180.0]


@pytest.fixture(scope="module")
def seg():
    p = capi.default_params(64, 64)
    p.max_batch = 1
    s = capi.Segmenter(p)
    yield s
    s.close()


def run(seg, pool, draws=None, indices=None, n=None, targets=None, ap="default", draws_given=True, counter=0, want_draws=True):
    """-> (out float32 [n][H][W][C], gathered targets or None, the draws buffer after the call or None); ap None = the validation loader"""
    _, H, W, C = pool.shape
    n = n if n is not None else (len(indices) if indices is not None else len(draws) if draws is not None else len(pool))
    d_pool = torch.from_numpy(pool).cuda()
    d_out = torch.full((n, H, W, C), -7.0, dtype=torch.float32, device="cuda")
    d_t = torch.from_numpy(np.asarray(targets, np.int32)).cuda() if targets is not None else None
    d_to = torch.full((n,), -7, dtype=torch.int32, device="cuda") if targets is not None else None
    d_draws = None
    if ap is not None and want_draws:
        host = draws if draws is not None else np.zeros(n, ref.DRAW_DTYPE)
        d_draws = torch.from_numpy(np.frombuffer(host.tobytes(), np.uint8).copy()).cuda()
    if isinstance(ap, str):
        ap = capi.default_augment_params(W, H)
    seg.augment_device(d_pool.data_ptr(), len(pool), n, W, H, C, d_out.data_ptr(), ap=ap, indices=indices,
                       d_pool_targets_ptr=d_t.data_ptr() if d_t is not None else 0, d_targets_out_ptr=d_to.data_ptr() if d_to is not None else 0,
                       d_draws_ptr=d_draws.data_ptr() if d_draws is not None else 0, draws_given=draws_given and ap is not None, counter=counter)
    seg.synchronize()
    back = np.frombuffer(d_draws.cpu().numpy().tobytes(), ref.DRAW_DTYPE) if d_draws is not None else None
    return d_out.cpu().numpy(), (d_to.cpu().numpy() if d_to is not None else None), back


def held_to_the_bar(name, dev, imgs, draws, extra=None):
    """device against (a) at 8 x E32 outside the band; extra = per-sample addition to the tolerance"""
    _, H, W, _ = imgs.shape
    a, b = ref.augment64(imgs, draws), ref.augment32(imgs, draws)
    keep = ~ref.band(draws, W, H)
    assert keep.mean() >= 0.99, f"{name}: the band excludes {100 * (1 - keep.mean()):.2f} % of the pixels, more than 1 %"
    e32 = float(np.abs(b - a)[keep].max())
    err = np.abs(dev.astype(np.float64) - a) * keep[..., None]
    tol = 8 * e32 + (np.zeros(len(draws)) if extra is None else extra)
    print(f"{name}: E32 = {e32:.3g}, bar = {8 * e32:.3g}, device max |d| = {err.max():.3g} over {len(draws)} samples ({100 * (1 - keep.mean()):.3f} % of the pixels in the band)")
    worst = err.reshape(len(draws), -1).max(axis=1)
    assert (worst <= tol).all(), f"{name}: sample {int(np.argmax(worst - tol))} is off by {worst.max():.3g}, bar {8 * e32:.3g}"


@pytest.mark.parametrize("W,H,C", SHAPES)
def test_validation_mode_is_float_of_byte_bit_for_bit(seg, W, H, C):
    pool = ref.sample_images(7, H, W, C, seed=11)
    targets = np.arange(7, dtype=np.int32) * 3 + 1
    rng = np.random.default_rng(5)
    for n in (1, 3, 130):
        if n == 130 and W == 256:
            continue                                                        # (100 MB of output says nothing the small sizes do not)
        idx = rng.integers(0, 7, n).astype(np.int32)
        out, t, _ = run(seg, pool, indices=idx, targets=targets, ap=None)
        assert out.tobytes() == ref.plain(pool[idx]).tobytes() and np.array_equal(t, targets[idx])
    out, t, _ = run(seg, pool, n=5, targets=targets, ap=None)                # indices NULL = 0 .. n-1
    assert out.tobytes() == ref.plain(pool[:5]).tobytes() and np.array_equal(t, targets[:5])
    out, _, _ = run(seg, pool, n=2, ap=None)                                 # without targets
    assert out.tobytes() == ref.plain(pool[:2]).tobytes()


@pytest.mark.parametrize("bad", [[0, 7, 1], [0, -1, 1]])
def test_an_index_outside_the_pool_is_refused_before_anything_runs(seg, bad):
    pool = ref.sample_images(7, 8, 8, 1, seed=11)
    d_pool = torch.from_numpy(pool).cuda()
    d_out = torch.full((3, 8, 8, 1), -7.0, dtype=torch.float32, device="cuda")
    for ap in (None, capi.default_augment_params(8, 8)):
        with pytest.raises(capi.TrexHipError) as e:
            seg.augment_device(d_pool.data_ptr(), 7, 3, 8, 8, 1, d_out.data_ptr(), ap=ap, indices=np.array(bad, np.int32))
        assert e.value.code == -1 and "indices[1]" in str(e.value)          # TREXHIP_E_INVALID
    with pytest.raises(capi.TrexHipError) as e:
        seg.augment_device(d_pool.data_ptr(), 7, 8, 8, 8, 1, d_out.data_ptr())       # 0 .. n-1 with n beyond the pool
    assert e.value.code == -1
    for w, h, c, code in ((7, 8, 1, -4), (8, 257, 1, -4), (8, 8, 2, -4)):
        with pytest.raises(capi.TrexHipError) as e:
            seg.augment_device(d_pool.data_ptr(), 1, 1, w, h, c, d_out.data_ptr())
        assert e.value.code == code
    seg.synchronize()
    assert bool((d_out == -7.0).all())


@pytest.mark.parametrize("W,H,C", SHAPES)
def test_geometry(seg, W, H, C):
    ap = capi.default_augment_params(W, H)
    ex, ey = int(round(ap.translate_x * W)), int(round(ap.translate_y * H))
    shifts = [(0, 0), (ex, ey), (-ex, -ey), (ex, -ey), (-ex, 0), (0, ey), (3, -3)]          # 0 and both extremes of the reference's range, and one beyond
    combos = [(a, s) for a in ANGLES for s in shifts] if W < 256 else [(a, shifts[i % len(shifts)]) for i, a in enumerate(ANGLES + ANGLES[1:5])]
    d = ref.make_draws(len(combos), angle=[c[0] for c in combos], tx=[c[1][0] for c in combos], ty=[c[1][1] for c in combos])
    pool = ref.sample_images(8, H, W, C, seed=21)
    idx = (np.arange(len(d)) * 3 + 7) % 8            # 7 = a random image first; every image meets several draws
    out, _, _ = run(seg, pool, draws=d, indices=idx.astype(np.int32))
    held_to_the_bar(f"geometry {W}x{H}x{C}", out, pool[idx], d)
    # the sign anchors on the device itself
    if W == H and W % 2 == 0:
        quarter = ref.make_draws(1, angle=90.0)
        out, _, _ = run(seg, pool[7:8], draws=quarter)
        assert np.abs(out[0] - np.rot90(pool[7], -1, axes=(0, 1))).max() < 1e-3


@pytest.mark.parametrize("W,H,C", SHAPES)
def test_values(seg, W, H, C):
    kinds = ref.value_draw_kinds()
    imgs, d = ref.value_cases(C, H, W, per_kind=2) if W < 256 else ref.value_cases(C, H, W, per_kind=1, kinds=kinds[::5])
    out, _, _ = run(seg, imgs, draws=d)
    assert not ref.band(d, W, H).any()                 # angle 0, whole shifts: exact geometry
    held_to_the_bar(f"values {W}x{H}x{C}", out, imgs, d)
    assert out.min() >= 0.0 and out.max() <= 255.0


@pytest.mark.parametrize("W,H,C,n", [(8, 8, 1, 130), (8, 8, 3, 130), (9, 11, 3, 130), (24, 24, 3, 130), (24, 24, 1, 3)])
def test_combined_where_the_band_is_empty(seg, W, H, C, n):
    d = ref.random_draws(n, W, H, seed=W + 31 * C, empty_band=True)
    pool = ref.sample_images(8, H, W, C, seed=23)
    idx = np.random.default_rng(3).integers(0, 8, n).astype(np.int32)
    out, _, _ = run(seg, pool, draws=d, indices=idx)
    assert not ref.band(d, W, H).any()
    held_to_the_bar(f"combined {W}x{H}x{C}", out, pool[idx], d)


@pytest.mark.parametrize("C", [1, 3])
def test_combined_at_80x80(seg, C):
    n, W, H = 32, 80, 80
    d = ref.random_draws(n, W, H, seed=41 + C)
    pool = ref.sample_images(8, H, W, C, seed=25)
    idx = (np.arange(n) % 8).astype(np.int32)
    out, _, _ = run(seg, pool, draws=d, indices=idx)
    # k band pixels that go the other way move the contrast mean by at most k / (H W) (values in [0, 1]), and through (1 - contrast) * mean
    # every pixel by at most 255 |1 - contrast| k / (H W): derived, not measured
    k = ref.band(d, W, H).sum(axis=(1, 2))
    held_to_the_bar(f"combined 80x80x{C}", out, pool[idx], d, extra=255.0 * np.abs(1.0 - d["contrast"].astype(np.float64)) * k / (H * W))


def test_determinism_and_independence_of_the_batch(seg):
    for (W, H, C, n) in ((80, 80, 3, 130), (9, 11, 3, 130), (256, 256, 3, 3)):
        d = ref.random_draws(n, W, H, seed=51)
        pool = ref.sample_images(8, H, W, C, seed=27)
        idx = np.random.default_rng(4).integers(0, 8, n).astype(np.int32)
        one, _, _ = run(seg, pool, draws=d, indices=idx)
        two, _, _ = run(seg, pool, draws=d, indices=idx)
        assert one.tobytes() == two.tobytes(), (W, H, C)
        for j in sorted({0, n // 2, n - 1}):
            alone, _, _ = run(seg, pool, draws=d[j:j + 1], indices=idx[j:j + 1])
            assert alone[0].tobytes() == one[j].tobytes(), (W, H, C, j)


def test_library_draws(seg):
    n, W, H, C = 4096, 8, 8, 3
    pool = ref.sample_images(8, H, W, C, seed=29)
    idx = (np.arange(n) % 8).astype(np.int32)
    ap = capi.default_augment_params(W, H, seed=1234)
    out, _, d = run(seg, pool, indices=idx, ap=ap, draws_given=False, counter=5)
    assert (np.abs(d["angle"]) <= 5.0).all() and abs(float(d["angle"].astype(np.float64).mean())) <= 0.27        # 6 sigma of U(-5, 5) over 4096
    assert d["angle"].min() < -4.5 and d["angle"].max() > 4.5
    for k, lo, hi in (("brightness", 0.85, 1.15), ("contrast", 0.85, 1.15), ("saturation", 0.85, 1.15), ("hue", -0.05, 0.05)):
        assert (d[k] >= np.float32(lo)).all() and (d[k] <= np.float32(hi)).all() and d[k].max() - d[k].min() > 0.9 * (hi - lo), k
    assert (np.abs(d["tx"]) <= round(ap.translate_x * W)).all() and (np.abs(d["ty"]) <= round(ap.translate_y * H)).all()
    orders = [tuple(ref.unpack_order(o)) for o in d["order"]]
    assert all(sorted(o) == [0, 1, 2, 3] for o in orders) and len(set(orders)) == 24 and (d["order"] >> 8 == 0).all()
    counts = np.unique(d["order"], return_counts=True)[1]
    assert counts.min() > 4096 / 24 - 6 * 13 and counts.max() < 4096 / 24 + 6 * 13          # binomial(4096, 1/24): sigma 12.8
    # the output is the reference run on the RETURNED draws
    held_to_the_bar("library draws 8x8x3", out, pool[idx], d)
    # the same (seed, counter) repeats -- also without a draws buffer --; another counter or seed differs
    out2, _, d2 = run(seg, pool, indices=idx, ap=ap, draws_given=False, counter=5)
    assert d2.tobytes() == d.tobytes() and out2.tobytes() == out.tobytes()
    out3, _, _ = run(seg, pool, indices=idx, ap=ap, draws_given=False, counter=5, want_draws=False)
    assert out3.tobytes() == out.tobytes()
    _, _, d4 = run(seg, pool, indices=idx, ap=ap, draws_given=False, counter=6)
    _, _, d5 = run(seg, pool, indices=idx, ap=capi.default_augment_params(W, H, seed=1235), draws_given=False, counter=5)
    assert (d4["angle"] != d["angle"]).mean() > 0.99 and (d5["angle"] != d["angle"]).mean() > 0.99
    # a wider translate range: whole pixels within +-round(translate * size), both ends reached
    wide = capi.default_augment_params(W, H, seed=7, translate_x=0.3, translate_y=0.2)
    out6, _, d6 = run(seg, pool, indices=idx, ap=wide, draws_given=False, counter=1)
    assert set(np.unique(d6["tx"])) == {-2, -1, 0, 1, 2} and set(np.unique(d6["ty"])) == {-2, -1, 0, 1, 2}          # +-2.4 and +-1.6, rounded
    held_to_the_bar("library draws 8x8x3, wide translate", out6, pool[idx], d6)


class Recorder:
    def __init__(self):
        self.batches, self.epochs, self.stop_training = [], [], False

    def on_batch_end(self, batch, logs):
        self.batches.append((batch, logs))

    def on_epoch_end(self, epoch, logs):
        self.epochs.append((epoch, logs))


def test_resident_training_learns(seg):
    from trex_amd import weights
    classes, n = 4, 32
    tr = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(classes, 9), classes), max_batch=n, lr=1e-3, seed=1)
    x, y = weights.synthetic_train_batch(n, 3, classes)                      # the 80 x 80 synthetic set of tests/test_train_loop.py's GPU test
    crops = np.rint(x).astype(np.uint8)
    train = train_loop.ResidentLoader(seg, np.concatenate([crops] * 3), np.concatenate([y] * 3), batch_size=n, seed=2)
    val = train_loop.ResidentLoader(seg, crops, y, batch_size=n, augment=False, shuffle=False)
    assert len(train) == 3 and len(val) == 1
    cb = Recorder()
    hist = train_loop.train_resident(tr, train, val, cb, train_loop.ReduceLROnPlateau(1e-3, patience=5), {"epochs": 6})
    print("resident training: val_loss per epoch", [round(h["val_loss"], 4) for h in hist], "loss", [round(h["loss"], 4) for h in hist])
    assert len(hist) == 6 and tr.steps == 6 * len(train) and len(cb.batches) == 18
    assert all(np.isfinite(h["loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    assert hist[-1]["val_loss"] < hist[0]["val_loss"]
    # what the loader last handed over is the validation batch, bit for bit
    got = seg.copy_to_host(val.d_inputs, (n, 80, 80, 1), np.float32)
    assert got.tobytes() == crops.astype(np.float32).tobytes() and np.array_equal(seg.copy_to_host(val.d_targets, (n,), np.int32), y)
    train.close(); val.close(); tr.close()
