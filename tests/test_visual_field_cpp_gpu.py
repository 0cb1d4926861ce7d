"""Builds and runs the C++ test of the visual-field adapter (tests/cpp/test_visual_field.cpp, trex_amd/host/HipVisualField.h) against the
library: HipVisualField::calculate through the C ABI equals cast_host and the Python restatement on the two-frame scene (5 and 12 entries)
and the others."""
import os
import subprocess
import pytest
import visual_field_scenes as S
from test_visual_field_cpp import write_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "test_visual_field_dev")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_visual_field.cpp"), "-o", exe,
           "-L", os.path.join(ROOT, "trex_amd"), "-ltrexhip", "-Wl,-rpath," + os.path.join(ROOT, "trex_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def test_visual_field_adapter_links_and_runs_its_host_side(tmp_path):
    # CPU-side: the whole header, calculate() included, is valid C++17 against the stand-in types and links against the ABI
    vec = str(tmp_path / "vectors.bin")
    write_vectors(vec, [S.scene("occlude3")[:2]])
    out = subprocess.run([build(tmp_path), vec], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "visual field host twin ok: 1 scenes" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_visual_field_adapter_equals_its_host_twin_on_the_device(tmp_path):
    vec = str(tmp_path / "vectors.bin")
    names = ("two_frames", "occlude3", "lds_exceed", "capacity")
    write_vectors(vec, [S.scene(n)[:2] for n in names])
    out = subprocess.run([build(tmp_path), vec, "--device"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"visual field adapter ok: {len(names)} scenes" in out.stdout, out.stdout + out.stderr
