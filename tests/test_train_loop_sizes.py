"""train_loop on a trainer whose individual_image_size is not 80x80, without a GPU: an epoch of train_resident over a fake trainer and a fake
context at 32 x 24, and the crop checks of ResidentValidation / ResidentAverages, which follow the trainer's size."""
import numpy as np
import pytest

from trex_amd import train_loop

W, H, CH, CLASSES = 32, 24, 1, 4


class FakeSeg:
    """device memory as counters; remembers what the loader asked the augmentation for"""

    def __init__(self):
        self.next, self.freed, self.calls = 4096, [], []

    def device_alloc(self, nbytes):
        p = self.next
        self.next += (int(nbytes) + 255) // 256 * 256
        return p

    def device_free(self, p):
        self.freed.append(p)

    def copy_to_device(self, d, arr):
        pass

    def augment_device(self, d_pool, pool, n, width, height, channels, d_out, **kw):
        self.calls.append((n, width, height, channels))


class FakeTrainer:
    classes, channels, width, height = CLASSES, CH, W, H

    def __init__(self):
        self.steps, self.evals, self.predicted = [], [], []

    def step_device(self, d_x, d_y, n, d_keep=0, want_loss=True):
        self.steps.append(n)
        return 1.0 / (1 + len(self.steps)), n // 2

    def evaluate_device(self, d_x, d_y, n):
        self.evals.append(n)
        return 0.5, n

    def predict_device(self, d_crops, n, d_probs):
        self.predicted.append(n)

    def set_lr(self, lr):
        pass


class Recorder:
    stop_training = False

    def __init__(self):
        self.batches, self.epochs = [], []

    def on_batch_end(self, batch, logs):
        self.batches.append(batch)

    def on_epoch_end(self, epoch, logs):
        self.epochs.append(logs)


def test_an_epoch_of_train_resident_at_32x24():
    seg, tr, cb = FakeSeg(), FakeTrainer(), Recorder()
    rng = np.random.default_rng(0)
    crops = rng.integers(0, 256, (10, H, W, CH), dtype=np.uint8)
    labels = rng.integers(0, CLASSES, 10)
    train = train_loop.ResidentLoader(seg, crops, labels, batch_size=4, seed=1)
    val = train_loop.ResidentLoader(seg, crops[:5], labels[:5], batch_size=4, augment=False, shuffle=False)
    assert (train.width, train.height, train.channels) == (tr.width, tr.height, tr.channels)
    hist = train_loop.train_resident(tr, train, val, cb, None, {"epochs": 1})
    assert tr.steps == [4, 4, 2] and tr.evals == [4, 1] and cb.batches == [0, 1, 2]
    assert seg.calls == [(4, W, H, CH), (4, W, H, CH), (2, W, H, CH), (4, W, H, CH), (1, W, H, CH)]
    assert len(hist) == 1 and hist[0]["val_acc"] == 1.0
    train.close()
    val.close()


def test_validation_and_averages_check_crops_against_the_trainers_size():
    seg, tr = FakeSeg(), FakeTrainer()
    good = np.zeros((6, H, W, CH), np.uint8)
    rv = train_loop.ResidentValidation(tr, seg, good, np.zeros(6, np.int64))
    assert (rv.height, rv.width, rv.n_val) == (H, W, 6)
    rv.close()
    for bad in (np.zeros((6, 80, 80, CH), np.uint8), np.zeros((6, W, H, CH), np.uint8), np.zeros((6, H, W, 3), np.uint8)):
        with pytest.raises(ValueError, match=f"{H}, {W}, {CH}"):
            train_loop.ResidentValidation(tr, seg, bad, np.zeros(6, np.int64))
        with pytest.raises(ValueError, match=f"{H}, {W}, {CH}"):
            train_loop.ResidentAverages(tr.predict_device, seg, bad, np.arange(6))
    ra = train_loop.ResidentAverages(tr.predict_device, seg, good, np.arange(6) % 2)
    assert ra.n == 6 and ra.classes == CLASSES
    ra.close()
