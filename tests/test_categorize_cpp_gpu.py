"""Builds and runs the C++ test of the categorisation adapter (tests/cpp/test_categorize.cpp, trex_amd/host/HipCategorize.h) through the C ABI:
predict against the labels of the Python wrapper, label_averaged on the device against its host twin."""
import os
import subprocess
import numpy as np
import pytest
from trex_amd import capi
import category_cases as cc
from test_categorize_cpp import ROOT, SOURCE, write_vectors


def build(tmp_path):
    exe = str(tmp_path / "test_categorize_dev")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), SOURCE, "-o", exe,
                           "-L", os.path.join(ROOT, "trex_amd"), "-ltrexhip", "-Wl,-rpath," + os.path.join(ROOT, "trex_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"])
    return exe


def test_categorize_adapter_compiles(tmp_path):
    # CPU-side: the header is valid C++17 and links against the ABI
    build(tmp_path)


@pytest.mark.gpu
def test_categorize_adapter_runs(tmp_path):
    exe = build(tmp_path)
    case = cc.CASES[2]                                   # 21 x 13 x 3, 70 categories
    crops = cc.crops(case, 37)
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_category_weights(cc.blob(case))
    labels = seg.categorize(crops)
    seg.close()
    assert np.array_equal(labels, cc.fixture()[f"case/{cc.case_id(case)}/labels/37"])
    votes, samples = write_vectors(str(tmp_path / "vectors.bin"))
    (tmp_path / "blob.bin").write_bytes(cc.blob(case))
    (tmp_path / "crops.bin").write_bytes(crops.tobytes())
    (tmp_path / "labels.bin").write_bytes(labels.astype("<i4").tobytes())
    out = subprocess.run([exe] + [str(tmp_path / f) for f in ("vectors.bin", "blob.bin", "crops.bin", "labels.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"categorize adapter ok: {votes} votes, {samples} samples, 37 crops" in out.stdout
