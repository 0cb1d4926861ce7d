"""tests/golden/cnn_trained_stats.npz: what the reference's own module learned on the stream of tests/identity_synth.py with three dropout
seeds (generator: tests/golden/make_trained_stats_fixture.py).  Checked here without a GPU: the recipe is learnable -- every reference run
counts as trained -- before any GPU time is spent on the device trainer's run of it (tests/test_cnn_trained_gpu.py)."""
import os
import numpy as np
import identity_synth
import trained_net

PATH = os.path.join(os.path.dirname(__file__), "golden", "cnn_trained_stats.npz")


def test_fixture_holds_three_trained_reference_runs():
    assert os.path.getsize(PATH) < 16 * 1024                        # numbers only: no weights
    z = np.load(PATH)
    assert [int(v) for v in z["meta"]] == [trained_net.CLASSES, trained_net.IDENTITY_SEED, trained_net.WEIGHT_SEED, trained_net.EPOCHS,
                                           identity_synth.BATCHES_PER_EPOCH, identity_synth.BATCH, trained_net.MONO_EPOCHS]
    h = z["history"]
    assert h.shape == (3, trained_net.EPOCHS, 3) and len(set(z["dropout_seeds"].tolist())) == 3
    assert z["test_accuracy"].shape == (3,) and z["test_top_softmax"].shape == (3,) and z["stage_quantiles"].shape == (3, 3, 3)
    assert np.all(np.isfinite(h))
    for r in range(3):
        assert z["test_accuracy"][r] >= trained_net.MIN_ACCURACY and z["test_top_softmax"][r] >= trained_net.MIN_TOP_SOFTMAX, r
        assert np.all(np.diff(h[r, :trained_net.MONO_EPOCHS, 0]) < 0), (r, h[r, :, 0])
        assert h[r, -1, 1] < 0.25 * h[r, 0, 1] and h[r, -1, 2] >= 0.9, r      # it learned: validation loss down, accuracy up
        q = z["stage_quantiles"][r]
        assert np.all(q > 0) and np.all(np.diff(q, axis=1) >= 0), r            # 50 <= 99 <= 100 %
    # the three runs drew different masks: they differ, and their spread is the yardstick of the device run
    assert np.ptp(h[:, -1, 1]) > 0
