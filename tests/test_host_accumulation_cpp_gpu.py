"""Builds and runs the C++ test of the accumulation adapter (tests/cpp/test_host_accumulation.cpp, trex_amd/host/HipAccumulation.h):
VINetwork::paverages reduced on the device over HipVINetwork through the C ABI, and the decision of check_additional_range on its result."""
import os
import subprocess
import pytest
from trex_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "test_host_accumulation")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_host_accumulation.cpp"), "-o", exe,
           "-L", os.path.join(ROOT, "trex_amd"), "-ltrexhip", "-Wl,-rpath," + os.path.join(ROOT, "trex_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def test_accumulation_adapter_compiles(tmp_path):
    # CPU-side: the header is valid C++17 against the stand-in types and links against the ABI
    build(tmp_path)


@pytest.mark.gpu
def test_accumulation_adapter_runs(tmp_path):
    exe = build(tmp_path)
    st = weights.synthetic_state(8, 77)
    crops = weights.synthetic_crops(48, 5)
    (tmp_path / "w.bin").write_bytes(weights.pack_blob(st, 8))
    (tmp_path / "c.bin").write_bytes(crops.tobytes())
    out = subprocess.run([exe, str(tmp_path / "w.bin"), str(tmp_path / "c.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "accumulation adapter ok" in out.stdout
