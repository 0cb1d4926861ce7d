"""Keeps the yardstick of the device augmentation honest (tests/augment_ref.py), on the CPU: the sign conventions of the affine map, the
identity, the torch float32 restatement (b) against the float64 formulas (a) -- geometry outside the near-tie band, values as E32 --, and
the host logic of train_loop.ResidentLoader / train_resident against recording stand-ins."""
import numpy as np
import pytest
import torch

import augment_ref as ref
from trex_amd import capi, train_loop

SIZES = [(8, 8), (9, 11), (50, 34), (80, 80), (256, 256)]           # (W, H)


def test_draw_record_is_the_abi_struct():
    assert ref.DRAW_DTYPE == capi.AUGMENT_DRAW_DTYPE and ref.IDENTITY_ORDER == capi.AUGMENT_IDENTITY_ORDER
    assert ref.unpack_order(ref.IDENTITY_ORDER) == [0, 1, 2, 3] and ref.pack_order([3, 0, 2, 1]) == 3 | 0 << 2 | 2 << 4 | 1 << 6


def test_params_struct_matches_the_header(tmp_path):
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "trexhip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",sizeof(trexhip_augment_params),'
                   'offsetof(trexhip_augment_params,seed),offsetof(trexhip_augment_params,hue_hi),sizeof(trexhip_augment_draw),offsetof(trexhip_augment_draw,order));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.AugmentParams), capi.AugmentParams.seed.offset, capi.AugmentParams.hue_hi.offset, capi.AUGMENT_DRAW_DTYPE.itemsize,
                   capi.AUGMENT_DRAW_DTYPE.fields["order"][1]]


def test_default_params_are_the_reference_transform():
    # visual_recognition_torch.py:1301 move_range = min(0.05, 2 / min(w, h)); :1325-1331 the transform
    p = capi.default_augment_params(80, 80)
    assert (p.degrees, p.translate_x, p.translate_y) == (5.0, np.float32(2 / 80), np.float32(2 / 80))
    assert [round(v, 6) for v in (p.brightness_lo, p.brightness_hi, p.contrast_lo, p.contrast_hi, p.saturation_lo, p.saturation_hi, p.hue_lo, p.hue_hi)] == \
        [0.85, 1.15, 0.85, 1.15, 0.85, 1.15, -0.05, 0.05]
    assert capi.default_augment_params(20, 30).translate_x == np.float32(0.05) and capi.default_augment_params(256, 100).translate_y == np.float32(0.02)


@pytest.mark.parametrize("fn", [ref.augment64, ref.augment32])
def test_sign_anchors(fn):
    rng = np.random.default_rng(1)
    img = rng.integers(1, 256, (1, 12, 12, 1), dtype=np.uint8)
    # angle 90 on an even square is np.rot90(img, -1): the angle turns clockwise
    got = fn(img, ref.make_draws(1, angle=90.0))
    assert np.allclose(got[0, :, :, 0], np.rot90(img[0, :, :, 0], -1), atol=1e-3)
    # tx = 1, ty = -2 moves the content one pixel right and two up; what comes in is 0
    got = fn(img, ref.make_draws(1, tx=1, ty=-2))[0, :, :, 0]
    want = np.zeros((12, 12))
    want[:-2, 1:] = img[0, 2:, :-1, 0]
    assert np.allclose(got, want, atol=1e-3)


@pytest.mark.parametrize("C", [1, 3])
def test_identity_draw_gives_the_image_back(C):
    img = ref.sample_images(8, 11, 9, C, seed=2)
    assert np.abs(ref.augment64(img, ref.make_draws(8)) - img).max() < 1e-9
    assert np.abs(ref.augment32(img, ref.make_draws(8)) - img).max() < 1e-3
    assert ref.plain(img).dtype == np.float32 and np.array_equal(ref.plain(img), img)
    # the validation loader's x.div(255).clamp(0, 1) * 255 (TRexImageDataset.__getitem__) returns every byte exactly in fp32
    b = torch.arange(256, dtype=torch.float32)
    assert torch.equal(b.div(255.0).clamp(0.0, 1.0) * 255.0, b)


@pytest.mark.parametrize("W,H", SIZES)
def test_geometry_of_the_fp32_restatement_equals_the_formulas_outside_the_band(W, H):
    # an "image" of pixel numbers 1 .. H*W (exact in fp32): a wrong source pixel is a wrong number
    n = 200
    d = ref.random_draws(n, W, H, seed=W * 1000 + H, translate=0.3, jitter=False)
    idx = np.broadcast_to(np.arange(1, H * W + 1, dtype=np.float32).reshape(1, H, W, 1), (n, H, W, 1))
    a = ref.affine64(idx, d)[..., 0]
    b = ref.affine32(torch.from_numpy(np.ascontiguousarray(idx)).permute(0, 3, 1, 2).contiguous(), d)[:, 0].numpy()
    band = ref.band(d, W, H)
    share = band.mean(axis=(1, 2))
    print(f"{W}x{H}: band holds {100 * band.mean():.3f} % of the pixels (largest sample {100 * share.max():.3f} %), "
          f"{int(((a != b) & ~band).sum())} mismatches outside it, {int(((a != b) & band).sum())} inside")
    assert band.mean() <= 0.01, "the band may exclude at most 1 % of a case's pixels"
    assert np.array_equal(a[~band], b[~band])


@pytest.mark.parametrize("C", [1, 3])
def test_e32_of_the_value_cases(C):
    imgs, d = ref.value_cases(C, 12, 10)
    a, b = ref.augment64(imgs, d), ref.augment32(imgs, d)
    e32 = float(np.abs(b - a).max())
    print(f"C = {C}: E32 = {e32:.3g} over {len(d)} value cases (units of [0, 255])")
    assert 0 < e32 < 1e-2          # fp32 against fp64 on values up to 255: a few ulp (1.5e-5 each), amplified by the hue round trip; not a wrong pixel or formula
    assert a.min() >= 0 and a.max() <= 255


# ---- ResidentLoader / train_resident against recording stand-ins ------------------------------------------------------------------------

class FakeSeg:
    """records what the loader asks of the context; "device memory" is a dict of numpy arrays keyed by a made-up address"""

    def __init__(self):
        self.mem, self.calls, self.freed, self.next = {}, [], [], 0x1000

    def device_alloc(self, nbytes):
        self.next += 0x100000
        self.mem[self.next] = None
        return self.next

    def device_free(self, p):
        self.freed.append(p)

    def copy_to_device(self, p, a):
        self.mem[p] = np.array(a)

    def augment_device(self, d_pool, pool_size, n, w, h, c, d_out, ap=None, indices=None, d_pool_targets_ptr=0, d_targets_out_ptr=0, d_draws_ptr=0,
                       draws_given=False, counter=0):
        self.calls.append(dict(pool=d_pool, pool_size=pool_size, n=n, shape=(h, w, c), out=d_out, ap=ap, indices=np.array(indices), pt=d_pool_targets_ptr,
                               to=d_targets_out_ptr, counter=counter))


def test_resident_loader_permutes_batches_and_keeps_the_last_partial_batch():
    seg = FakeSeg()
    x = np.random.default_rng(0).integers(0, 256, (10, 8, 9, 1), dtype=np.uint8)
    y = np.arange(10) % 3
    ld = train_loop.ResidentLoader(seg, x, y, batch_size=4, seed=7)
    assert len(ld) == 3 and np.array_equal(seg.mem[ld.d_pool], x) and seg.mem[ld.d_pool_targets].dtype == np.int32
    epochs = []
    for _ in range(2):
        got = list(ld)
        assert [g[2] for g in got] == [4, 4, 2] and all(g[:2] == (ld.d_inputs, ld.d_targets) for g in got)       # drop_last=False
        epochs.append(np.concatenate([c["indices"] for c in seg.calls[-3:]]))
    assert all(sorted(e) == list(range(10)) for e in epochs) and not np.array_equal(epochs[0], epochs[1])        # a new permutation per epoch
    assert np.array_equal(epochs[0], ld.order(0)) and np.array_equal(epochs[1], ld.order(1))
    c = seg.calls[0]
    assert c["shape"] == (8, 9, 1) and c["pool_size"] == 10 and c["pt"] == ld.d_pool_targets and c["to"] == ld.d_targets and c["indices"].dtype == np.int32
    assert c["ap"].seed == 7 and c["ap"].degrees == 5.0 and [k["counter"] for k in seg.calls] == list(range(6))   # new draws for every call
    again = train_loop.ResidentLoader(FakeSeg(), x, y, batch_size=4, seed=7)
    assert np.array_equal(again.order(0), epochs[0]) and not np.array_equal(train_loop.ResidentLoader(FakeSeg(), x, y, 4, seed=8).order(0), epochs[0])
    ld.close()
    assert sorted(seg.freed) == sorted(seg.mem)
    # the validation loader: in order, no transform; a pool that is already on the device is used where it is
    seg2 = FakeSeg()
    val = train_loop.ResidentLoader(seg2, 0xABC000, 0xDEF000, batch_size=8, augment=False, shuffle=False, count=10, image_shape=(8, 9, 3))
    assert [g[2] for g in val] == [8, 2] and np.array_equal(np.concatenate([c["indices"] for c in seg2.calls]), np.arange(10))
    assert all(c["ap"] is None and c["pool"] == 0xABC000 and c["pt"] == 0xDEF000 and c["shape"] == (8, 9, 3) for c in seg2.calls)
    val.close()
    assert 0xABC000 not in seg2.freed and 0xDEF000 not in seg2.freed
    with pytest.raises(ValueError):
        train_loop.ResidentLoader(FakeSeg(), x.astype(np.float32), y, 4)
    with pytest.raises(ValueError):
        train_loop.ResidentLoader(FakeSeg(), x, y.astype(np.float32), 4)


class FakeDeviceTrainer:
    def __init__(self):
        self.calls, self.lrs = [], []

    def step_device(self, d_x, d_y, n):
        self.calls.append(("step", d_x, d_y, n))
        return 1.0 / (1 + len(self.calls)), n // 2

    def evaluate_device(self, d_x, d_y, n):
        self.calls.append(("eval", d_x, d_y, n))
        return 0.5, n

    def set_lr(self, lr):
        self.lrs.append(lr)


class Recorder:
    def __init__(self, stop_after=None):
        self.batches, self.epochs, self.stop_training, self.stop_after = [], [], False, stop_after

    def on_batch_end(self, batch, logs):
        self.batches.append((batch, logs))

    def on_epoch_end(self, epoch, logs):
        self.epochs.append((epoch, logs))
        if self.stop_after is not None and epoch >= self.stop_after:
            self.stop_training = True


def test_train_resident_is_the_epoch_loop_of_train():
    x = np.zeros((10, 8, 8, 1), np.uint8)
    y = np.arange(10) % 3
    tl, vl = train_loop.ResidentLoader(FakeSeg(), x, y, 4), train_loop.ResidentLoader(FakeSeg(), x[:5], y[:5], 4, augment=False, shuffle=False)
    tr, cb = FakeDeviceTrainer(), Recorder(stop_after=2)
    hist = train_loop.train_resident(tr, tl, vl, cb, train_loop.ReduceLROnPlateau(1e-3, patience=0), {"epochs": 10})
    assert len(hist) == 3 and len(cb.batches) == 9 and [c[0] for c in tr.calls[:5]] == ["step"] * 3 + ["eval"] * 2
    assert [c[3] for c in tr.calls[:5]] == [4, 4, 2, 4, 1] and tr.calls[0][1:3] == (tl.d_inputs, tl.d_targets) and tr.calls[3][1:3] == (vl.d_inputs, vl.d_targets)
    assert cb.batches[2][1]["acc"] == 0.5 and cb.epochs[0][1]["val_acc"] == 1.0 and set(cb.epochs[0][1]) == {"val_loss", "val_acc", "val_precision", "val_recall"}
    assert len(tr.lrs) == 3 and tr.lrs[1] == pytest.approx(1e-4)
    tr2, cb2 = FakeDeviceTrainer(), Recorder()
    hist2 = train_loop.train_resident(tr2, tl, [], cb2, None, {"epochs": 5}, abort=lambda: len(cb2.epochs) >= 2)
    assert len(hist2) == 2 and set(cb2.epochs[0][1]) == {"loss", "acc"} and not tr2.lrs
