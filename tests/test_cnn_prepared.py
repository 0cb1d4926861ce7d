"""The record trexhip_identify_prepare_device leaves and the rule by which the next identify call may skip the prepared launches
(trex_amd/csrc/cnn_prepared.h), on the CPU: tests/cpp/test_cnn_prepared.cpp runs each check below against the header the library compiles.
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_prepared") / ("test_cnn_prepared_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_prepared.cpp"), "-o", path])
    return path


@pytest.mark.parametrize("check", ["match", "fields", "one_shot", "dropped"])
def test_record(exe, check):
    """match: the call a record was made for finds it; fields: crops, n, mode, geometry word, stream and either generation differing in turn
    do not, and take the record with them; one_shot: consumed twice, replaced, prepared twice; dropped: by loading weights, a precision
    change, a reallocated batch and closing, the first and third starting a new generation"""
    r = subprocess.run([exe, check], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr and r.stdout.strip() == check + " ok", r.stdout + r.stderr
