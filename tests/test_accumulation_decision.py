"""Builds and runs tests/cpp/test_accumulation_decision.cpp on the CPU: track::decide_additional_range (trex_amd/host/HipAccumulation.h),
the restatement of Accumulation::check_additional_range's decision (ui/Accumulation.cpp:520-640), on cases worked out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decide_additional_range_on_hand_worked_cases(tmp_path):
    exe = str(tmp_path / "test_accumulation_decision")
    # no library on the link line: the decision is pure host code
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_accumulation_decision.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "accumulation decision ok" in out.stdout, out.stdout + out.stderr
