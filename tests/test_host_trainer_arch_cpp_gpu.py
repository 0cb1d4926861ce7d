"""Builds and runs the C++ test of HipVINetwork::Trainer on a v100 blob (tests/cpp/test_host_trainer_arch.cpp, trex_amd/host/HipVINetwork.h):
train_batch, evaluate and weights() round tripping through HipVINetwork::load_weights, through the C ABI."""
import os
import subprocess
import pytest
from trex_amd import weights
import train_arch_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "test_host_trainer_arch")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_host_trainer_arch.cpp"), "-o", exe,
           "-L", os.path.join(ROOT, "trex_amd"), "-ltrexhip", "-Wl,-rpath," + os.path.join(ROOT, "trex_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def test_trainer_adapter_compiles(tmp_path):
    # CPU-side: the header is valid C++17 against the stand-in types and links against the ABI (trexhip_trainer_version included)
    build(tmp_path)


@pytest.mark.gpu
def test_trainer_adapter_trains_a_v100_network(tmp_path):
    exe = build(tmp_path)
    W, H, classes = 24, 16, 5
    case = ((W, H, 1, 12, classes), 5100, "adapter")
    (tmp_path / "w.bin").write_bytes(weights.pack_blob(tc.initial_state(case, "v100"), classes, 1, W, H, "v100"))
    (tmp_path / "c.bin").write_bytes(tc.crops(case, 12, 9).tobytes())
    out = subprocess.run([exe, str(tmp_path / "w.bin"), str(tmp_path / "c.bin"), str(W), str(H), str(classes)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "v100 trainer facade ok" in out.stdout
