"""The host twin of the tracklet vote and sample_rows (trex_amd/host/HipCategorize.h) against vectors written by the Python restatement
(tests/category_ref.py), byte for byte.  Plain g++, no library, no device; built once more with the address and undefined-behaviour sanitizers
(a stand-alone program)."""
import os
import struct
import subprocess
import numpy as np
import category_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_categorize.cpp")


def vote_cases():
    """(labels, tracklet, T, C): the hand cases of test_category_ref.py and random rows with labels that are none (negative) and out of range"""
    cases = [([2, 0, 2, 0, -1, 5, 1], [1, 1, 1, 1, 1, 1, 3], 4, 3), ([-1, -1, 9], [0, 0, 0], 1, 3), ([], [], 3, 2), ([0], [0], 1, 1),
             ([1, 0, 1, 0, 2, 2], [0, 1, 0, 1, 0, 1], 2, 3)]
    for seed, (n, T, C) in enumerate([(1, 1, 1), (500, 7, 4), (3000, 1, 70), (3000, 900, 2), (2000, 5, 1024)]):
        rng = np.random.default_rng(seed)
        cases.append((rng.integers(-2, C + 2, n).tolist(), rng.integers(0, T, n).tolist(), T, C))
    return cases


def sample_cases():
    """(size, first_frame, sample_rate, min_samples)"""
    out = [(size, first, 50, 20) for size in (1, 14, 15, 16, 19, 20, 21, 100, 1234) for first in (0, 3, 5, 9, 1000)]
    out += [(size, 7, 3, 5) for size in (4, 5, 6, 15, 40)] + [(300, 10, 1000, 20), (18, 4, 50, 10)]
    return out


def write_vectors(path):
    votes, samples = vote_cases(), sample_cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(votes)))
        for labels, tracklet, T, C in votes:
            counts, rows, label, share, skipped = cr.vote(labels, tracklet, T, C)
            f.write(struct.pack("<3i", len(labels), T, C))
            for a, dt in ((labels, "<i4"), (tracklet, "<i4"), (counts, "<u4"), (rows, "<u4"), (label, "<i4"), (share, "<f4")):
                f.write(np.ascontiguousarray(a, dt).tobytes())
            f.write(struct.pack("<I", skipped))
        f.write(struct.pack("<i", len(samples)))
        for size, first, rate, min_samples in samples:
            rows, valid = cr.sample_rows(size, first, rate, min_samples)
            f.write(struct.pack("<4q2i", size, first, rate, min_samples, len(rows), int(valid)))
            f.write(np.ascontiguousarray(rows, "<i4").tobytes())
    return len(votes), len(samples)


def build_host_only(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-DTREXHIP_CATEGORIZE_HOST_ONLY", *extra, SOURCE, "-o", exe])
    return exe


def test_host_twin_equals_the_restatement(tmp_path):
    vec = str(tmp_path / "vectors.bin")
    votes, samples = write_vectors(vec)
    out = subprocess.run([build_host_only(tmp_path, "test_categorize"), vec], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"categorize host twin ok: {votes} votes, {samples} samples" in out.stdout, out.stdout + out.stderr


def test_host_twin_under_the_sanitizers(tmp_path):
    vec = str(tmp_path / "vectors.bin")
    write_vectors(vec)
    exe = build_host_only(tmp_path, "test_categorize_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "categorize host twin ok" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
