"""Synthetic identities for training the identity network at test time (TEST INFRASTRUCTURE ONLY; a plain module, imported by the tests
and by tests/golden/make_trained_stats_fixture.py).

A deterministic numpy recipe (PCG64: the same bits wherever numpy runs).  `Identities(classes, seed)` draws, per identity and seeded per
identity, a fixed body -- an ellipse with a round head at one end -- and a fixed texture: a base grey value plus three plane waves in
body coordinates.  Rendering turns the body by a random angle, shifts it by a few pixels, multiplies by a brightness gain and adds pixel
noise, on black, in the style of trex_amd.weights.synthetic_crops.  What tells two identities apart (size, aspect, grey level, texture
frequencies) survives all of that, so a few hundred optimizer steps learn it; pose, gain and noise keep it from being memorised.

Three disjoint seed ranges: the training stream (float32 in [0, 255], NOT integer, as weights.synthetic_train_batch documents for the
reference's augmented loader), the validation set and the test set (uint8, what the tracker hands over).
"""
import numpy as np

SIZE = 80
TRAIN_SEED, VAL_SEED, TEST_SEED, TILE_SEED = 1 << 20, 2 << 20, 3 << 20, 4 << 20     # disjoint ranges of render seeds
BATCH = 128
BATCHES_PER_EPOCH = 16
N_VAL = 512
N_TEST = 2048
_CHUNK = 1024


class Identities:
    def __init__(self, classes=16, seed=0):
        self.classes, self.seed = int(classes), int(seed)
        p = {k: [] for k in ("a", "b", "head", "hr", "base", "amp", "fu", "fv", "ph")}
        for k in range(self.classes):
            rng = np.random.default_rng([self.seed, k])                    # seeded per identity: identity k is the same in any class count
            a, b = rng.uniform(14.0, 30.0), rng.uniform(5.0, 11.0)
            p["a"].append(a); p["b"].append(b)
            p["head"].append(a * rng.uniform(0.45, 0.75)); p["hr"].append(b * rng.uniform(0.9, 1.4))
            p["base"].append(rng.uniform(70.0, 180.0))
            p["amp"].append(rng.uniform(15.0, 40.0, 3))
            p["fu"].append(rng.uniform(-0.9, 0.9, 3)); p["fv"].append(rng.uniform(-0.9, 0.9, 3))
            p["ph"].append(rng.uniform(0.0, 2 * np.pi, 3))
        self.p = {k: np.asarray(v, np.float32) for k, v in p.items()}

    def render(self, labels, seed):
        """labels: (n,) identity indices -> float32 (n, 80, 80, 1) in [0, 255], not rounded."""
        labels = np.asarray(labels, np.int64)
        n = labels.shape[0]
        rng = np.random.default_rng([self.seed, 0x5eed, int(seed)])
        th = rng.uniform(0.0, 2 * np.pi, n).astype(np.float32)
        cx = (SIZE / 2 - 0.5 + rng.uniform(-3.0, 3.0, n)).astype(np.float32)
        cy = (SIZE / 2 - 0.5 + rng.uniform(-3.0, 3.0, n)).astype(np.float32)
        gain = rng.uniform(0.8, 1.2, n).astype(np.float32)
        out = np.empty((n, SIZE, SIZE, 1), np.float32)
        yy, xx = np.mgrid[0:SIZE, 0:SIZE].astype(np.float32)
        for lo in range(0, n, _CHUNK):
            s = slice(lo, min(lo + _CHUNK, n))
            m = s.stop - s.start
            noise = rng.standard_normal((m, SIZE, SIZE), np.float32) * np.float32(4.0)
            q = {k: v[labels[s]] for k, v in self.p.items()}
            c, si = np.cos(th[s])[:, None, None], np.sin(th[s])[:, None, None]
            X, Y = xx[None] - cx[s][:, None, None], yy[None] - cy[s][:, None, None]
            u, v = X * c + Y * si, Y * c - X * si
            e = lambda name: q[name][:, None, None]
            mask = ((u / e("a")) ** 2 + (v / e("b")) ** 2 <= 1.0) | ((u - e("head")) ** 2 + v ** 2 <= e("hr") ** 2)
            tex = np.broadcast_to(e("base"), u.shape).copy()
            for k in range(3):
                tex += q["amp"][:, k, None, None] * np.sin(q["fu"][:, k, None, None] * u + q["fv"][:, k, None, None] * v + q["ph"][:, k, None, None])
            img = np.clip(tex * gain[s][:, None, None] + noise, 1.0, 255.0) * mask
            out[s, :, :, 0] = img
        return out

    def render_u8(self, labels, seed):
        return np.rint(self.render(labels, seed)).astype(np.uint8)

    def sample(self, identity, n, seed):
        """n crops of one identity: uint8 (n, 80, 80, 1)."""
        return self.render_u8(np.full(n, identity, np.int64), seed)

    def _labels(self, n, seed):
        """balanced labels in a seeded order"""
        rng = np.random.default_rng([self.seed, 0x1abe1, int(seed)])
        return rng.permutation(np.arange(n) % self.classes).astype(np.int32)

    # ---- the three sets -------------------------------------------------------------------------------------------------------------
    def train_epoch(self, epoch, batches=BATCHES_PER_EPOCH, batch=BATCH):
        """the training stream: epoch `epoch` is `batches` fresh batches of (float32 (batch, 80, 80, 1) in [0, 255], int32 labels)"""
        out = []
        for i in range(batches):
            s = TRAIN_SEED + int(epoch) * batches + i
            y = self._labels(batch, s)
            out.append((self.render(y, s), y))
        return out

    def validation_set(self, n=N_VAL):
        y = self._labels(n, VAL_SEED)
        return self.render_u8(y, VAL_SEED), y

    def test_set(self, n=N_TEST):
        y = self._labels(n, TEST_SEED)
        return self.render_u8(y, TEST_SEED), y

    def tiled_set(self, n, tile=N_TEST):
        """n crops: the test set's labels tiled, every tile with pose / gain / noise seeds of its own"""
        y0 = self._labels(tile, TEST_SEED)
        xs, ys = [], []
        for t, lo in enumerate(range(0, n, tile)):
            m = min(tile, n - lo)
            xs.append(self.render_u8(y0[:m], TILE_SEED + t)); ys.append(y0[:m])
        return np.concatenate(xs), np.concatenate(ys)


def edge_crops(ids, identity=3):
    """the crops no training stream holds: all-zero, all-255, one identity at 0.2x and 2x brightness (clipped), uniform noise"""
    base = ids.render(np.full(4, identity, np.int64), TEST_SEED + 99)
    rng = np.random.default_rng([ids.seed, 0xed6e])
    out = [np.zeros((1, SIZE, SIZE, 1), np.uint8), np.full((1, SIZE, SIZE, 1), 255, np.uint8),
           np.rint(np.clip(base * 0.2, 0, 255)).astype(np.uint8), np.rint(np.clip(base * 2.0, 0, 255)).astype(np.uint8),
           rng.integers(0, 256, (4, SIZE, SIZE, 1)).astype(np.uint8)]
    return np.concatenate(out)


def unseen_crops():
    """full frames the trained statistics never saw: saturated 255, and 255 / 0 checkerboards at periods 1, 2 and 5 (both phases)"""
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    out = [np.full((SIZE, SIZE), 255, np.uint8)]
    for p in (1, 2, 5):
        cb = (((yy // p) + (xx // p)) % 2).astype(np.uint8) * 255
        out += [cb, 255 - cb]
    return np.stack(out)[..., None]
