"""Builds and runs the C++ test of the prefilter adapter (tests/cpp/test_prefilter.cpp, trex_amd/host/HipPrefilter.h): the shape / bdx
packing on the host, and Tracker::prefilter's per-frame lists through the C ABI on the device."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "test_prefilter")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_prefilter.cpp"), "-o", exe,
           "-L", os.path.join(ROOT, "trex_amd"), "-ltrexhip", "-Wl,-rpath," + os.path.join(ROOT, "trex_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def test_prefilter_adapter_compiles_and_packs(tmp_path):
    # CPU-side: the header is valid C++17 against the stand-in types, links against the ABI, and packs the tables as documented
    out = subprocess.run([build(tmp_path), "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "prefilter packing ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_prefilter_adapter_runs(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "prefilter adapter ok" in out.stdout
