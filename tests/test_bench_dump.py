"""bench.py --dump-outputs: what the last timed step handed its caller goes to DIR/<name>.npy in float32 / float64, every value exact,
64 MB at most (a fixed, seeded sample of rows beyond that).  CPU-only: the writer is driven with a stand-in lane whose tables live in
host memory, laid out as the library's pinned tables and the ID table are."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from trex_amd import capi, dist as tdist  # noqa: E402


def _lane(n_blobs, n_runs, n_pixels, classes, posture, seed=1):
    """two frames, frame 1 first in the pooled tables (the kernels take the frames' offsets with atomics)"""
    rng = np.random.default_rng(seed)
    info = np.zeros(2, capi.INFO_DTYPE)
    for f, n in (("blob", n_blobs), ("run", n_runs), ("pix", n_pixels)):
        info["n_" + f + ("els" if f == "pix" else "s")] = [n // 3, n - n // 3]
        info[f + "_begin"] = [n - n // 3, 0]
    blobs = np.zeros(n_blobs, capi.BLOB_DTYPE)
    for f in ("run_begin", "n_pixels", "bid", "px_min_max"):
        blobs[f] = rng.integers(0, 2 ** 32, n_blobs, dtype=np.uint64)
    blobs["m20"] = rng.integers(0, 2 ** 50, n_blobs, dtype=np.uint64)
    runs = np.zeros(n_runs, capi.RUN_DTYPE)
    runs["x0"], runs["y"] = rng.integers(0, 65536, n_runs), rng.integers(0, 65536, n_runs)
    pixels = rng.integers(0, 256, n_pixels, dtype=np.uint8)
    res = capi.BatchResult()
    res.n_frames, res.total_blobs, res.total_runs, res.total_pixels = len(info), n_blobs, n_runs, n_pixels
    res.frames, res.blobs, res.runs, res.pixels = info.ctypes.data, blobs.ctypes.data, runs.ctypes.data, pixels.ctypes.data
    res.pixel_channels = 1
    hdr = tdist.HDR_EX if posture else tdist.HDR
    rowlen = hdr + classes + (75 if posture else 0)
    table = np.zeros((n_blobs + 7, rowlen), np.int32)
    table[:n_blobs, :hdr] = rng.integers(0, 2 ** 31, (n_blobs, hdr))
    table[:n_blobs, 5:7] = rng.standard_normal((n_blobs, 2)).astype(np.float32).view(np.int32)
    if posture:
        table[:n_blobs, 8:15] = rng.standard_normal((n_blobs, 7)).astype(np.float32).view(np.int32)
    table[:n_blobs, 0] = np.repeat([1, 0], [n_blobs - n_blobs // 3, n_blobs // 3])       # global frame index, pooled order
    table[:n_blobs, 7] = 1
    table[:n_blobs, hdr:] = rng.random((n_blobs, rowlen - hdr), dtype=np.float32).view(np.int32)
    ln = types.SimpleNamespace(res=res, n=n_blobs, table_host=torch.from_numpy(table), keep=(info, blobs, runs, pixels))
    if posture:
        ln.p_mid = torch.from_numpy(rng.random((n_blobs + 3, 25, 4), dtype=np.float32))
        minfo = np.zeros((n_blobs + 3, 8), np.int32)
        minfo[:, 0] = rng.integers(0, 3, n_blobs + 3)
        ln.p_minfo = torch.from_numpy(minfo)
    pipe = types.SimpleNamespace(with_posture=posture, with_cnn=True, classes=classes)
    return pipe, ln, (info, blobs, runs, pixels, table)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _frame_order(a, n):
    return np.concatenate([a[n - n // 3:], a[:n - n // 3]])          # frame 0's entries, then frame 1's


def test_small_step_is_written_whole_exact_and_frame_by_frame(tmp_path):
    pipe, ln, (info, blobs, runs, pixels, table) = _lane(300, 2000, 9000, 8, posture=False)
    bench.dump_outputs(str(tmp_path), pipe, ln)
    got = _load(str(tmp_path))
    assert set(got) == {"frames", "blobs", "runs", "pixels", "id_header", "probs"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    names = list(capi.BLOB_DTYPE.names)
    for f in ("bid", "m20"):
        assert np.array_equal(got["blobs"][:, names.index(f)], _frame_order(blobs[f], 300).astype(np.float64))
    assert np.array_equal(got["runs"][:, 0], _frame_order(runs["x0"], 2000)) and got["runs"].shape == (2000, 3)
    assert np.array_equal(got["pixels"][:, 0], _frame_order(pixels, 9000))
    assert np.array_equal(got["frames"][:, 0], info["n_blobs"]) and got["frames"].shape == (2, 6)      # without the pooled offsets
    valid = _frame_order(table[:300], 300)
    assert np.array_equal(got["id_header"][:, 0], [0] * 100 + [1] * 200)
    assert np.array_equal(got["probs"], valid[:, 8:].view(np.float32))
    assert np.array_equal(got["id_header"][:, 1], valid[:, 1].astype(np.float64))
    assert np.array_equal(got["id_header"][:, 5:7], valid[:, 5:7].view(np.float32).astype(np.float64))


def test_posture_rows_without_a_midline_are_zero(tmp_path):
    pipe, ln, _ = _lane(200, 100, 100, 4, posture=True)
    bench.dump_outputs(str(tmp_path), pipe, ln)
    got = _load(str(tmp_path))
    status = _frame_order(ln.p_minfo[:200, 0].numpy(), 200)
    mid = _frame_order(ln.p_mid[:200].flatten(1).numpy(), 200)
    assert got["midline"].shape == (200, 100) and not got["midline"][status != 0].any()
    assert np.array_equal(got["midline"][status == 0], mid[status == 0])
    assert np.array_equal(got["midline_info"][:, 0], status) and got["id_midline"].shape == (200, 75)


def test_a_large_step_is_cut_to_a_fixed_sample_under_64_mb(tmp_path):
    pipe, ln, (_, _, _, pixels, _) = _lane(40000, 300000, 20_000_000, 100, posture=False)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), pipe, ln)
    bench.dump_outputs(str(b), pipe, ln)
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= bench.DUMP_BYTES
    got, again = _load(str(a)), _load(str(b))
    assert set(got) == set(again) and all(np.array_equal(got[k], again[k]) for k in got)
    rows = got["pixels_rows"].astype(np.int64)
    assert np.array_equal(got["pixels"][:, 0], _frame_order(pixels, len(pixels))[rows]) and (np.diff(rows) > 0).all()
