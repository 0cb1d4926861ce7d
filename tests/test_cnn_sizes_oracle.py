"""individual_image_size other than 80x80 on the host: the CPU oracle against the reference's own network at those sizes
(tests/golden/cnn_v118_3_sizes.npz; generator: tests/golden/make_cnn_size_fixtures.py), and the weight blob / checkpoint
conversion at those sizes."""
import importlib.util
import os
import numpy as np
import pytest
import torch
from oracle import cnn_oracle
from trex_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cnn_v118_3_sizes.npz")
CASES = [tuple(int(x) for x in row) for row in np.load(GOLD)["cases"]]      # (W, H, CH, classes, seed)


def case_id(case):
    return f"{case[0]}x{case[1]}x{case[2]}"


def load_size_case(case):
    """-> (fixture, state with the calibrated running statistics, {n: (probs, logits)}, {n: crops})"""
    w, h, ch, classes, seed = case
    z = np.load(GOLD)
    pre = f"case/{case_id(case)}/"
    st = weights.synthetic_state(classes, seed, ch, w, h)
    for k in z.files:
        if k.startswith(pre + "stat/"):
            st[k[len(pre) + 5:]] = z[k]
    ns = sorted(int(k.split("/")[-1]) for k in z.files if k.startswith(pre + "probs/"))
    want = {n: (z[pre + f"probs/{n}"], z[pre + f"logits/{n}"]) for n in ns}
    crops = {n: weights.synthetic_crops(n, seed + 1000 + n, ch, w, h) for n in ns}
    return st, want, crops


def test_fixture_covers_the_cases_of_the_issue():
    sizes = {(w, h, ch) for w, h, ch, _, _ in CASES}
    assert {(64, 64, 1), (96, 96, 1), (128, 128, 1), (100, 60, 1), (52, 52, 3), (8, 8, 1)} <= sizes


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_matches_reference_vectors_at_other_sizes(case):
    st, want, crops = load_size_case(case)
    for n, (probs, logits) in want.items():
        p, lg = cnn_oracle.predict(st, crops[n], threads=8)
        assert p.shape == probs.shape
        assert np.abs(p - probs).max() <= 1e-5, (n, np.abs(p - probs).max())
        assert np.abs(lg - logits).max() <= 2e-3


def test_blob_round_trip_non_square():
    st = weights.synthetic_state(8, 3, 1, 100, 60)
    assert st["fc1.weight"].shape == (100, 128 * (100 // 8) * (60 // 8))
    blob = weights.pack_blob(st, 8, 1, 100, 60)
    assert np.frombuffer(blob[:32], np.int32)[3:6].tolist() == [100, 60, 1]
    back, classes, channels = weights.unpack_blob(blob)
    assert (classes, channels) == (8, 1)
    assert all(np.array_equal(back[k], st[k]) for k in st)


def test_convert_reads_input_shape():
    spec = importlib.util.spec_from_file_location("convert_weights", os.path.join(ROOT, "tools", "convert_weights.py"))
    cw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cw)
    st = weights.synthetic_state(8, 5, 1, 64, 64)
    ck = {"model": None, "state_dict": {"model." + k: torch.from_numpy(v) for k, v in st.items()},
          "metadata": {"input_shape": (64, 64, 1), "num_classes": 8, "model_type": "v118_3"}}
    blob, c, w, h, ch = cw.convert(ck)
    assert (c, w, h, ch) == (8, 64, 64, 1)
    assert blob == weights.pack_blob(st, 8, 1, 64, 64)
