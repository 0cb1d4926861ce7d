"""Pins the CNN oracle (own restatement) on vectors produced by importing the reference's network
(tests/golden/cnn_v118_3_*.npz; generator: tests/golden/make_cnn_fixtures.py).  Tolerance 1e-4 abs on
softmax (BASELINE.json north_star), 2e-3 abs on logits (|logit| up to ~15)."""
import os
import numpy as np
import pytest
import torch
from oracle import cnn_oracle
from trex_amd import weights

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load_fixture(classes):
    z = np.load(os.path.join(GOLD, f"cnn_v118_3_c{classes}.npz"))
    st = weights.synthetic_state(int(z["classes"]), int(z["seed"]))
    for k in z.files:
        if k.startswith("stat/"):
            st[k[5:]] = z[k]
    return z, st


@pytest.mark.parametrize("classes", [8, 100, 256])
def test_oracle_matches_reference_vectors(classes):
    z, st = load_fixture(classes)
    sizes = sorted(int(k.split("/")[1]) for k in z.files if k.startswith("probs/"))
    for n in sizes[:3]:
        crops = weights.synthetic_crops(n, int(z["seed"]) + 1000 + n)
        probs, logits = cnn_oracle.predict(st, crops, threads=8)
        assert np.abs(probs - z[f"probs/{n}"]).max() <= 1e-4
        assert np.abs(logits - z[f"logits/{n}"]).max() <= 2e-3
        assert np.allclose(probs.sum(1), 1.0, atol=1e-5)


@pytest.mark.parametrize("classes", [8, 100, 256])
def test_float64_oracle_matches_reference_vectors(classes):
    """the float64 reading is pinned by the same outside vectors as the float32 one, ten times closer: the reference's stored softmax is an
    fp32 result, and double arithmetic on the same weights lies within 1e-5 of it.  Logits come back as float64."""
    z, st = load_fixture(classes)
    sizes = sorted(int(k.split("/")[1]) for k in z.files if k.startswith("probs/"))
    for n in sizes[:3]:
        crops = weights.synthetic_crops(n, int(z["seed"]) + 1000 + n)
        probs, logits = cnn_oracle.predict(st, crops, threads=8, dtype=torch.float64)
        assert probs.dtype == np.float64 and logits.dtype == np.float64
        err = float(np.abs(probs - z[f"probs/{n}"]).max())
        print(f"classes {classes}, {n} crops: max |float64 softmax - reference softmax| = {err:.3g}")
        assert err <= 1e-5, (n, err)
        assert np.abs(logits - z[f"logits/{n}"]).max() <= 2e-3
        assert np.allclose(probs.sum(1), 1.0, atol=1e-12)
        # the default stays what it was: float32 in, float32 out, and the two readings agree to fp32 rounding
        p32, l32 = cnn_oracle.predict(st, crops, threads=8)
        assert p32.dtype == np.float32 and l32.dtype == np.float32
        assert np.abs(p32 - probs).max() <= 1e-5


def test_stage_maxima_are_the_forward_passes_own_activations():
    """stage_maxima: per crop the largest activation behind each conv + BN + ReLU + pool stage.  An empty crop's first stage is max(0, folded
    bias) over the channels; scaling bn1's affine by f scales the first stage by f; both dtypes agree to fp32 rounding"""
    z, st = load_fixture(8)
    crops = weights.synthetic_crops(6, 3)
    crops[2] = 0
    m64 = cnn_oracle.stage_maxima(st, crops)
    m32 = cnn_oracle.stage_maxima(st, crops, dtype=torch.float32)
    assert len(m64) == 3 and all(m.shape == (6,) and m.dtype == np.float64 for m in m64) and all(m.dtype == np.float32 for m in m32)
    for a, b in zip(m64, m32):
        assert np.all(a >= 0) and np.abs(a - b).max() <= 1e-4 * max(1.0, a.max())
    s = st["bn1.weight"].astype(np.float64) / np.sqrt(st["bn1.running_var"].astype(np.float64) + cnn_oracle.EPS_BN)
    folded = (st["conv1.bias"].astype(np.float64) - st["bn1.running_mean"]) * s + st["bn1.bias"]
    assert abs(m64[0][2] - max(folded.max(), 0.0)) <= 1e-12 * max(1.0, abs(folded).max())
    st2 = dict(st); st2["bn1.weight"] = st["bn1.weight"] * np.float32(4.0); st2["bn1.bias"] = st["bn1.bias"] * np.float32(4.0)
    assert np.allclose(cnn_oracle.stage_maxima(st2, crops)[0], 4.0 * m64[0], rtol=1e-12)


def test_batch_rule_and_transform_results():
    assert [cnn_oracle.batch_size_rule(n) for n in (1, 8, 64, 65, 100, 128, 1024)] == [64, 64, 64, 128, 128, 128, 128]
    vals = np.arange(6, dtype=np.float32).reshape(2, 3)
    flat = cnn_oracle.transform_results(4, [2, 0], vals)
    assert flat.tolist() == [3, 4, 5, -1, -1, -1, 0, 1, 2, -1, -1, -1]


def test_blob_roundtrip():
    st = weights.synthetic_state(8, 1)
    blob = weights.pack_blob(st, 8)
    assert len(blob) == 32 + 4 * sum(int(np.prod(s)) for _, s in weights.shapes(8))
