"""The host twin of the visual-field rule (HipVisualField::cast_host, trex_amd/host/HipVisualField.h) against vectors written by the Python
restatement: the hand-worked cases of tests/test_visual_field_ref.py and every scene of tests/visual_field_scenes.py, byte for byte.
Plain g++, no library, no device; built once more with the address and undefined-behaviour sanitizers (a stand-alone program)."""
import os
import struct
import subprocess
import numpy as np
import pytest
import visual_field_ref as R
import visual_field_scenes as S
import test_visual_field_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pack(a, want):
    rows, max_points = a["outline"].shape[:2]
    head = struct.pack("<6i2d", rows, max_points, len(a["frame_entries"]) - 1, len(a["entries"]), len(a["observers"]), int(a["max_tess"]),
                       float(a["max_d"]), float(a["max_distance"]))
    parts = [a["outline"].astype("<f4"), a["info"], a["frame_entries"].astype("<i4"), a["entries"], a["observers"],
             want["depth"], want["ids"], want["points"], want["fov"], want["head_distance"], want["status"]]
    return head + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def hand_case(sc, max_d, max_distance=1000.0, max_tess=64):
    """a scene of tests/test_visual_field_ref.py in the layout of the generated ones"""
    info = np.zeros(len(sc["n_outline"]), S.INFO_DTYPE)
    info["n_outline"], info["tail_index"], info["head_index"] = sc["n_outline"], sc["tail_index"], sc["head_index"]
    a = dict(outline=sc["outline"], info=info, frame_entries=sc["frame_entries"], entries=sc["entries"], observers=sc["observers"], max_d=max_d,
             max_distance=max_distance, max_tess=max_tess)
    return a, S.reference(a)


def hand_cases():
    sq, behind = H.SQUARE, H.BEHIND
    unused = H.scene([(1, behind, 0, (0, 0)), (7, sq, 0, (100, 0)), (8, sq, -1, (60, 0)), (9, sq, 0, (50, 0))])
    unused["entries"]["posture_row"][3] = -1
    no_self = {k: v.copy() for k, v in unused.items()}
    no_self["entries"]["flags"][0] = 1
    return [
        hand_case(H.scene([(1, behind, 0, (0, 0)), (7, sq, 0, (100, 0))]), 40400.0),
        hand_case(H.scene([(1, behind, 0, (0, 0)), (7, sq, 0, (100, 0)), (8, sq, 0, (200, 0))]), 404000.0),
        hand_case(H.scene([(1, behind, 0, (0, 0)), (8, sq, 0, (200, 0)), (7, sq, 0, (100, 0))]), 404000.0),
        hand_case(H.scene([(8, sq, 0, (200, 0)), (7, sq, 0, (100, 0)), (1, sq, 0, (50, 0))], observer=2), 404000.0),
        hand_case(H.scene([(1, behind, 0, (0, 0)), (7, sq, 0, (-120, 0))]), 40400.0),
        hand_case(H.scene([(1, [(10, 1), (10, -1), (12, 0)], 0, (0, 0)), (7, [(0, -10), (-10, -10), (-10, 10), (0, 10)], 0, (-100, 0))], eye_angle=np.pi), 40400.0),
        hand_case(H.scene([(1, behind, 0, (0, 0)), (7, [(-50, 87), (-77, 64)], 0, (0, 0))]), 1e12),
        hand_case(H.scene([(1, behind, 0, (0, 0)), (7, H.NEAR_THEN_FAR, 2, (0, 0))]), 1e12),                       # left_side == 0: head distance -inf
        hand_case(H.scene([(1, [(-10, 1), (-10, -1), (-11, -1), (-12, -1), (-13, 0), (-12, 1), (-11, 1), (-10.5, 1)], 5, (0, 0)),
                           (7, H.NEAR_THEN_FAR, 0, (0, 0))]), 1e12),                                               # the observer's tail index in hd
        hand_case(unused, 40400.0, 5.0, 12),                                                                         # tessellated, skipped entries
        hand_case(unused, 40400.0, 5.0, 11),                                                                         # status 2
        hand_case(no_self, 40400.0),                                                                                 # status 1
    ]


def write_vectors(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for a, want in cases:
            f.write(pack(a, want))


def all_cases():
    return hand_cases() + [S.scene(n)[:2] for n in S.NAMES]


def build_host_only(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-DTREXHIP_VF_HOST_ONLY", *extra, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_visual_field.cpp"), "-o", exe])
    return exe


def test_every_scene_is_free_of_fragile_records():
    # visual_field_scenes.scene() refuses a scene with one fragile record; building them all here is the CPU check of the seeds
    for n in S.NAMES:
        a, want, rep = S.scene(n)
        assert rep["fragile"] == []
        assert len(want["status"]) == len(a["observers"])
    statuses = [int(s) for c in hand_cases() for s in c[1]["status"]]
    assert statuses.count(1) == 1 and statuses.count(2) == 1


def test_layouts_agree_with_the_wrapper():
    from trex_amd import capi
    assert capi.VF_ENTRY_DTYPE == R.ENTRY_DTYPE and capi.VF_OBSERVER_DTYPE == R.OBSERVER_DTYPE and capi.POSTURE_INFO_DTYPE == S.INFO_DTYPE
    assert (capi.VF_CHUNK_RECORDS, capi.VF_LDS_RECORDS) == (S.CHUNK_RECORDS, S.LDS_RECORDS)
    assert capi.VfParams.max_points.offset == 16 and capi.VfParams.max_tess_points.offset == 20


def test_host_twin_equals_the_restatement(tmp_path):
    vec = str(tmp_path / "vectors.bin")
    cases = all_cases()
    write_vectors(vec, cases)
    out = subprocess.run([build_host_only(tmp_path, "test_visual_field"), vec], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"visual field host twin ok: {len(cases)} scenes" in out.stdout, out.stdout + out.stderr


def test_host_twin_under_the_sanitizers(tmp_path):
    vec = str(tmp_path / "vectors.bin")
    cases = all_cases()
    write_vectors(vec, cases)
    exe = build_host_only(tmp_path, "test_visual_field_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    out = subprocess.run([exe, vec], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "visual field host twin ok" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
