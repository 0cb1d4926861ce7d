"""Builds and runs the C++ test of HipCategorize::Trainer (tests/cpp/test_categorize_trainer.cpp, trex_amd/host/HipCategorize.h) through the C ABI:
three steps with library-drawn masks, an evaluation, the export and load_into + predict, against the Python wrapper's own run with the same seed --
the library is deterministic, so losses, counts, labels and the exported blob are equal bit for bit."""
import os
import subprocess
import numpy as np
import pytest
from trex_amd import capi
import category_train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_categorize_trainer.cpp")


def build(tmp_path):
    exe = str(tmp_path / "test_categorize_trainer")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SOURCE, "-o", exe,
                           "-L", os.path.join(ROOT, "trex_amd"), "-ltrexhip", "-Wl,-rpath," + os.path.join(ROOT, "trex_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return exe


def test_categorize_trainer_compiles(tmp_path):
    # CPU-side: the header is valid C++17 and links against the ABI
    build(tmp_path)


@pytest.mark.gpu
def test_categorize_trainer_runs(tmp_path):
    exe = build(tmp_path)
    case = tc.find(21, 13)
    W, H, ch, n, categories = case[0]
    from trex_amd import weights
    blob = weights.pack_category_blob(tc.initial_state(case), categories, ch, W, H)
    x, y, _ = tc.inputs(case)
    crops = tc.crops(case, 9, 4)
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    tr = capi.Trainer(seg, blob, max_batch=n, lr=1e-4, dropout=0.25, precision=1, seed=5)
    steps = [tr.step(x, y) for _ in range(3)]
    ev = tr.evaluate(x, y)
    exported = tr.export()
    tr.close()
    seg.load_category_weights(exported)
    labels = seg.categorize(crops)
    seg.close()
    for name, data in (("blob.bin", blob), ("x.bin", x.tobytes()), ("y.bin", y.astype("<i4").tobytes()), ("crops.bin", crops.tobytes())):
        (tmp_path / name).write_bytes(data)
    out = subprocess.run([exe] + [str(tmp_path / f) for f in ("blob.bin", "x.bin", "y.bin", "crops.bin", "out.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"categorize trainer ok: {n} samples, 9 crops" in out.stdout
    got = (tmp_path / "out.bin").read_bytes()
    want = (np.array([s[0] for s in steps], "<f4").tobytes() + np.array([s[1] for s in steps], "<i4").tobytes() + np.array([ev[0]], "<f4").tobytes() +
            np.array([ev[1]], "<i4").tobytes() + labels.astype("<i4").tobytes() + exported)
    assert got == want
