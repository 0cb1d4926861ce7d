"""Builds and runs the C++ test of the tracklet-images adapter (tests/cpp/test_host_tracklet_images.cpp, trex_amd/host/HipTrackletImages.h):
the median image per tracklet of Export.cpp:1287-1364 reduced on the device through the C ABI, against the adapter's line-by-line host twin."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "test_host_tracklet_images")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_host_tracklet_images.cpp"), "-o", exe,
           "-L", os.path.join(ROOT, "trex_amd"), "-ltrexhip", "-Wl,-rpath," + os.path.join(ROOT, "trex_amd"),
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def test_tracklet_images_adapter_compiles_and_its_host_twin_is_the_sorted_median(tmp_path):
    # CPU-side: the header is valid C++17 against the stand-in types and links against the ABI; the host twin needs no device
    exe = build(tmp_path)
    out = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tracklet images adapter ok: host twin" in out.stdout


@pytest.mark.gpu
def test_tracklet_images_adapter_runs(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tracklet images adapter ok: device route = host twin" in out.stdout
