"""tests/identity_synth.py: the synthetic identities the trained-network tests are built on."""
import time
import numpy as np
import identity_synth
from identity_synth import Identities


def test_recipe_is_deterministic_and_seeded_per_identity():
    a, b = Identities(16, 7), Identities(16, 7)
    x = a.sample(5, 12, 3)
    assert x.dtype == np.uint8 and x.shape == (12, 80, 80, 1)
    assert np.array_equal(x, b.sample(5, 12, 3))
    assert not np.array_equal(x, a.sample(5, 12, 4))              # another pose seed
    assert not np.array_equal(x, a.sample(6, 12, 3))              # another identity, same poses
    assert not np.array_equal(x, Identities(16, 8).sample(5, 12, 3))
    for k in a.p:                                                  # identity k does not depend on how many identities there are
        assert np.array_equal(a.p[k][:4], Identities(4, 7).p[k])
    assert x[:, 30:50, 30:50].any() and (x[:, 0] == 0).all() and (x[:, :, 0] == 0).all()      # a body in the middle, black at the border


def test_crops_look_like_blobs_on_black_and_identities_differ():
    ids = Identities(16, 7)
    x, y = ids.test_set(512)
    assert x.shape == (512, 80, 80, 1) and np.array_equal(np.bincount(y), np.full(16, 32))
    area = (x > 0).reshape(512, -1).mean(1)
    assert 0.02 < area.min() and area.max() < 0.45
    assert x.max() > 150
    # something simple already tells many identities apart (area and mean grey of the body): the recipe is learnable
    feat = np.stack([area * 100, np.array([c[c > 0].mean() for c in x]) / 10], 1)
    cent = np.stack([feat[y == k].mean(0) for k in range(16)])
    guess = ((feat[:, None] - cent[None]) ** 2).sum(2).argmin(1)
    assert (guess == y).mean() > 0.3, (guess == y).mean()


def test_training_stream_is_float_and_the_sets_are_disjoint():
    ids = Identities(16, 7)
    ep = ids.train_epoch(0, batches=2)
    assert len(ep) == 2
    x, y = ep[0]
    assert x.dtype == np.float32 and x.shape == (128, 80, 80, 1) and y.dtype == np.int32 and y.shape == (128,)
    assert x.min() >= 0.0 and x.max() <= 255.0
    assert np.abs(x - np.rint(x)).max() > 0.1                     # not integer: the gain is not
    assert np.array_equal(np.bincount(y), np.full(16, 8))
    assert not np.array_equal(x, ep[1][0]) and not np.array_equal(ids.train_epoch(1, batches=1)[0][0], x)
    assert np.array_equal(ids.train_epoch(0, batches=1)[0][0], x)
    vx, vy = ids.validation_set(128)
    tx, ty = ids.test_set(128)
    assert vx.dtype == np.uint8 and tx.dtype == np.uint8
    assert not np.array_equal(vx, tx) and not np.array_equal(np.rint(x).astype(np.uint8), vx) and not np.array_equal(np.rint(x).astype(np.uint8), tx)
    t, ty2 = ids.tiled_set(300, tile=128)
    assert t.shape == (300, 80, 80, 1) and np.array_equal(ty2[:128], ty2[128:256]) and not np.array_equal(t[:128], t[128:256])


def test_rendering_a_few_thousand_crops_takes_seconds():
    t0 = time.time()
    x, _ = Identities(16, 7).test_set(4096)
    dt = time.time() - t0
    assert x.shape[0] == 4096 and dt < 30.0, dt


def test_edge_and_unseen_crops():
    e = identity_synth.edge_crops(Identities(16, 7))
    assert e.dtype == np.uint8 and e.shape[1:] == (80, 80, 1)
    assert (e[0] == 0).all() and (e[1] == 255).all()
    dim, bright = e[2:6].astype(np.float64), e[6:10].astype(np.float64)
    assert 0 < dim.max() <= 52 and (bright == 255).mean() > 0.02 and bright.sum() > 4 * dim.sum()
    u = identity_synth.unseen_crops()
    assert u.dtype == np.uint8 and u.shape == (7, 80, 80, 1) and set(np.unique(u)) == {0, 255}
    assert (u[0] == 255).all()
    for k, p in ((1, 1), (3, 2), (5, 5)):
        c = u[k, :, :, 0]
        assert np.array_equal(c, 255 - u[k + 1, :, :, 0])
        assert (c[:p, :p] == c[0, 0]).all() and c[0, p] != c[0, 0] and c[p, 0] != c[0, 0] and c[p, p] == c[0, 0]
