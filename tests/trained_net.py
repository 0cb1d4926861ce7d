"""A TRAINED identity network, made at test time by the project's own trainer (TEST INFRASTRUCTURE ONLY; a plain module).

trained_state() starts from weights.synthetic_state and runs train_loop.train on a capi.Trainer over the stream of
tests/identity_synth.py: default precision, library-drawn dropout masks with a fixed seed, Adam at lr 1e-3, ReduceLROnPlateau, batches of
128, EPOCHS epochs.  Weights are not committed: fc1.weight alone is 5 MB of incompressible floats, and the device trainer makes them in
seconds.  They are only INPUTS: everything the tests assert about them is computed by the float64 oracle from the same weights.

The same recipe, run on the reference's own module with three dropout seeds, is tests/golden/make_trained_stats_fixture.py ->
tests/golden/cnn_trained_stats.npz.
"""
import functools
import numpy as np
import torch

from oracle import cnn_oracle
from trex_amd import capi, train_loop, weights
import identity_synth

CLASSES = 16
IDENTITY_SEED = 7
WEIGHT_SEED = 2024
DROPOUT_SEED = 12345
LR = 1e-3
EPOCHS = 20
MONO_EPOCHS = 5            # the training loss falls from epoch to epoch over these first epochs (asserted of the reference runs by the generator)
MIN_ACCURACY = 0.95        # "trained": the float64 oracle classifies at least this share of the held-out test set correctly ...
MIN_TOP_SOFTMAX = 0.9      # ... and its mean top softmax there is at least this


class _Quiet:
    stop_training = False

    def on_batch_end(self, batch, logs):
        pass

    def on_epoch_end(self, epoch, logs):
        pass


def identities(classes=CLASSES):
    return identity_synth.Identities(classes, IDENTITY_SEED)


class _Stream:
    """train loader: a fresh epoch of the stream every time the loop iterates over it"""

    def __init__(self, ids):
        self.ids, self.epoch = ids, 0

    def __len__(self):
        return identity_synth.BATCHES_PER_EPOCH

    def __iter__(self):
        e, self.epoch = self.epoch, self.epoch + 1
        return iter(self.ids.train_epoch(e))


def _train(classes, seed, precision):
    ids = identities(classes)
    vx, vy = ids.validation_set()
    vx = vx.astype(np.float32)
    B = identity_synth.BATCH
    val = [(vx[lo:lo + B], vy[lo:lo + B]) for lo in range(0, len(vy), B)]
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    tr = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(classes, WEIGHT_SEED), classes), max_batch=B, lr=LR, seed=seed, precision=precision)
    sched = train_loop.ReduceLROnPlateau(LR, mode="min", factor=0.1, patience=5)
    history = train_loop.train(tr, _Stream(ids), val, _Quiet(), sched, {"epochs": EPOCHS})
    blob = tr.export()
    tr.close(); seg.close()
    return blob, history


@functools.lru_cache(maxsize=None)
def trained_blob(classes=CLASSES, seed=DROPOUT_SEED, precision=0):
    """-> (weight blob as trexhip_load_weights takes it, history of train_loop.train); trained at most once per process and argument set"""
    return _train(classes, seed, precision)


def trained_state(classes=CLASSES, seed=DROPOUT_SEED, precision=0):
    """-> (state dict name -> float32 ndarray, history)"""
    blob, history = trained_blob(classes, seed, precision)
    st, c, ch = weights.unpack_blob(blob)
    assert c == classes and ch == 1
    return st, history


def oracle_f64(st, crops, chunk=256, threads=16):
    """float64 oracle in chunks -> (softmax, logits), both float64"""
    ps, ls = [], []
    for lo in range(0, len(crops), chunk):
        p, l = cnn_oracle.predict(st, crops[lo:lo + chunk], threads=threads, dtype=torch.float64)
        ps.append(p); ls.append(l)
    return np.concatenate(ps), np.concatenate(ls)


def oracle_f32_logits(st, crops, chunk=512, threads=16):
    return np.concatenate([cnn_oracle.forward_logits(st, crops[lo:lo + chunk], threads=threads) for lo in range(0, len(crops), chunk)])


def stage_maxima(st, crops, dtype=torch.float32, chunk=512, threads=16):
    parts = [cnn_oracle.stage_maxima(st, crops[lo:lo + chunk], dtype=dtype, threads=threads) for lo in range(0, len(crops), chunk)]
    return [np.concatenate([p[k] for p in parts]) for k in range(3)]


@functools.lru_cache(maxsize=None)
def held_out_reference(classes=CLASSES, seed=DROPOUT_SEED):
    """the held-out test set through the float64 oracle on the trained weights: (crops, labels, softmax, logits), computed once per process"""
    st, _ = trained_state(classes, seed)
    x, y = identities(classes).test_set()
    p, l = oracle_f64(st, x)
    return x, y, p, l


def assert_trained(classes=CLASSES, seed=DROPOUT_SEED):
    """the preconditions of every test on the trained net: if the recipe misses them, lengthen it -- the bar stays"""
    x, y, p, l = held_out_reference(classes, seed)
    acc, top = float((p.argmax(1) == y).mean()), float(p.max(1).mean())
    assert acc >= MIN_ACCURACY and top >= MIN_TOP_SOFTMAX, f"the net does not count as trained: test accuracy {acc:.4f}, mean top softmax {top:.4f}"
    return acc, top
