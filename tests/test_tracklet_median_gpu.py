"""Every tracklet's crops reduced to its median image on the device: trexhip_tracklet_medians_device against tests/tracklet_median_ref.py
(hist_utils::addImage and the loop of Export.cpp:1287-1364, line by line), byte for byte.  Counts from 255 up are held to final_median --
the same walk applied once to the finished histograms; tests/test_tracklet_median_ref.py shows it equal to the walk per image at 255, 256
and 257."""
import functools

import numpy as np
import pytest
import torch

import tracklet_median_ref as R
from tracklet_median_cases import constructed
from trex_amd import capi, synth

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4
FILL_MED, FILL_ROWS = 0xA5, 0xDEADBEEF


@pytest.fixture(scope="module")
def seg():
    p = capi.default_params(64, 64)
    p.max_batch = 1
    s = capi.Segmenter(p)
    yield s
    s.close()


def device_call(seg, crops, tracklet, T, off=0, shape=None):
    """crops uint8 (n, H, W, C), tracklet int (n,) on the host -> (medians (T, H, W), rows (T,), bytes around the median buffer untouched).
    off: d_crops and d_median stand that many bytes behind a 256-byte aligned address"""
    crops = np.ascontiguousarray(crops, np.uint8)
    n = crops.shape[0]
    H, W, C = shape if shape is not None else crops.shape[1:]
    d_crops = torch.zeros(crops.size + off + 16, dtype=torch.uint8, device="cuda")
    d_crops[off:off + crops.size] = torch.from_numpy(crops.reshape(-1)).cuda()
    d_tr = torch.from_numpy(np.ascontiguousarray(tracklet, np.int32)).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_med = torch.full((T * H * W + off + 16,), FILL_MED, dtype=torch.uint8, device="cuda")
    d_rows = torch.from_numpy(np.full(T, FILL_ROWS, np.uint32).view(np.int32)).cuda()
    assert d_crops.data_ptr() % 256 == 0 and d_med.data_ptr() % 256 == 0
    seg.tracklet_medians_device(d_crops.data_ptr() + off, n, W, H, C, d_tr.data_ptr(), T, d_med.data_ptr() + off, d_rows.data_ptr())
    seg.synchronize()
    med = d_med.cpu().numpy()
    guard_ok = (med[:off] == FILL_MED).all() and (med[off + T * H * W:] == FILL_MED).all()
    return med[off:off + T * H * W].reshape(T, H, W), d_rows.cpu().numpy().view(np.uint32), bool(guard_ok)


def refused(seg, crops, tracklet, T, shape=None):
    """-> the error; asserts that the call left both output buffers as they were"""
    crops = np.ascontiguousarray(crops, np.uint8)
    n = crops.shape[0]
    H, W, C = shape if shape is not None else crops.shape[1:]
    d_crops = torch.from_numpy(crops.reshape(-1)).cuda() if crops.size else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_tr = torch.from_numpy(np.ascontiguousarray(tracklet, np.int32)).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    d_med = torch.full((max(T, 1) * 256 * 256,), FILL_MED, dtype=torch.uint8, device="cuda")
    d_rows = torch.from_numpy(np.full(max(T, 1), FILL_ROWS, np.uint32).view(np.int32)).cuda()
    with pytest.raises(capi.TrexHipError) as e:
        seg.tracklet_medians_device(d_crops.data_ptr(), n, W, H, C, d_tr.data_ptr(), T, d_med.data_ptr(), d_rows.data_ptr())
    seg.synchronize()
    assert bool((d_med == FILL_MED).all()) and (d_rows.cpu().numpy().view(np.uint32) == FILL_ROWS).all(), "a refused call wrote output"
    return e.value


def layout(counts, rng, strays=3):
    """tracklet ids for tracklets of the given sizes, interleaved at random, with rows of no tracklet (-1) scattered in"""
    tr = np.concatenate([np.full(c, t, np.int32) for t, c in enumerate(counts)] + [np.full(strays, -1, np.int32)])
    return tr[rng.permutation(len(tr))]


# ---- 1. shapes: the minimum, a ragged dword tile, odd sizes on the byte path, the flagship size, the maximum; aligned and one byte off ----
SHAPES = [(8, 8, 1), (9, 8, 1), (13, 11, 3), (13, 11, 1), (80, 80, 1), (80, 80, 3)]          # (W, H, C)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("W,H,C", SHAPES)
def test_shapes_and_small_counts(seg, W, H, C, off):
    rng = np.random.default_rng(W * 1000 + H * 10 + C)
    counts = [3, 0, 1, 4, 2, 9, 0]                                      # tracklets 1 and 6 (the last) have no rows
    tr = layout(counts, rng)
    crops = rng.integers(0, 256, (len(tr), H, W, C), dtype=np.uint8)
    crops[tr == 5] = (crops[tr == 5] >> 5) + 0x60                       # values 0x60..0x67: one high nibble, the low one decides
    want, want_rows = R.medians(crops, tr, len(counts))
    got, rows, guard = device_call(seg, crops, tr, len(counts), off)
    assert rows.tolist() == counts and np.array_equal(rows, want_rows)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert guard, "bytes outside d_median were written"
    assert not got[1].any() and not got[6].any()                        # the image init leaves
    assert np.array_equal(got[2], R.to_gray(crops[tr == 2][0]))         # one row gives the image (its gray) back


@functools.lru_cache(maxsize=None)
def largest_case():
    crops = np.random.default_rng(256).integers(0, 256, (5, 256, 256, 3), dtype=np.uint8)
    tr = np.zeros(5, np.int32)
    return crops, tr, R.medians(crops, tr, 1)[0]


@pytest.mark.parametrize("off", [0, 1])
def test_largest_size_five_rows(seg, off):
    crops, tr, want = largest_case()
    got, rows, guard = device_call(seg, crops, tr, 1, off)
    assert rows.tolist() == [5] and guard and np.array_equal(got, want)


# ---- 2. counts around a counter of 8 bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,C", [(9, 8, 1), (13, 11, 3)])
def test_counts_255_256_257(seg, W, H, C):
    rng = np.random.default_rng(W)
    counts = [255, 256, 257]
    tr = layout(counts, rng, strays=5)
    crops = rng.integers(0, 256, (len(tr), H, W, C), dtype=np.uint8)
    if C == 1:                                                          # tracklet 1: every image the same -- one bin holds 256
        crops[tr == 1] = rng.integers(0, 256, (1, H, W, C), dtype=np.uint8)
    want, _ = R.medians(crops, tr, 3, incremental=False)
    got, rows, guard = device_call(seg, crops, tr, 3)
    assert rows.tolist() == counts and guard and np.array_equal(got, want)


# ---- 3. the count limit: a bin at 32767, its packed neighbour sees no carry --------------------------------------------------------------
def test_32767_equal_bytes(seg):
    m = R.MAX_ROWS
    # every image the same; the pixels walk through both halves of a packed counter pair, in the high and in the low nibble
    img = np.array([0x00, 0x0f, 0x10, 0x1f, 0xe0, 0xef, 0xf0, 0xff] * 8, np.uint8).reshape(1, 8, 8, 1)
    img[0, 7, :, 0] = [0x5a, 0xa5, 0x7f, 0x80, 0x01, 0xfe, 0x11, 0xee]
    crops = np.repeat(img, m, axis=0)
    got, rows, guard = device_call(seg, crops, np.zeros(m, np.int32), 1)
    hist = np.zeros((8, 8, 256), np.int32)
    np.put_along_axis(hist, img[0].astype(np.int64), m, axis=2)
    assert np.array_equal(R.final_median(hist, np.full((8, 8), m)), img[0, :, :, 0])
    assert rows.tolist() == [m] and guard and np.array_equal(got[0], img[0, :, :, 0])


def test_32767_split_between_two_values(seg):
    m = R.MAX_ROWS
    a = np.array([3, 250, 0x40, 0x4f, 0, 255, 0x7f, 0x80], np.uint8)    # 16383 images hold a, 16384 hold b, alternating
    b = np.array([250, 3, 0x4f, 0x40, 255, 0, 0x80, 0x7f], np.uint8)
    crops = np.empty((m, 8, 8, 1), np.uint8)
    crops[0::2] = b[None, None, :, None]
    crops[1::2] = a[None, None, :, None]
    hist = np.zeros((8, 8, 256), np.int32)
    for x in range(8):
        hist[:, x, a[x]], hist[:, x, b[x]] = m // 2, m - m // 2
    want = R.final_median(hist, np.full((8, 8), m))
    # rank 16383: behind 16383 smaller values it is the first b (the walk goes on past a), inside 16384 smaller values it is the last b
    assert np.array_equal(want[0], b)
    got, rows, guard = device_call(seg, crops, np.zeros(m, np.int32), 1)
    assert rows.tolist() == [m] and guard and np.array_equal(got[0], want)


# ---- 4. values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 3, 4, 16, 33])
def test_constructed_values(seg, m):
    """all 0, all 255, half 0 / half 255 (255 at an even count), one high nibble, the first and the last low nibble of a high nibble, random"""
    stack = constructed(m)                                              # (m, 2, 8)
    crops = np.zeros((m, 8, 8, 1), np.uint8)
    crops[:, :2, :, 0] = stack
    crops[:, 2:4, :, 0] = stack[::-1]                                   # the same stacks in the other order
    crops[:, 4:, :, 0] = np.random.default_rng(m).integers(0, 256, (m, 4, 8))
    tr = np.zeros(m, np.int32)
    want, _ = R.medians(crops, tr, 1)
    got, rows, guard = device_call(seg, crops, tr, 1)
    assert guard and np.array_equal(got, want)
    assert got[0, 0, 0] == 0 and got[0, 0, 1] == 255 and got[0, 0, 2] == 255 and got[0, 0, 6] == 0x30 and got[0, 0, 7] == 0x3f
    assert np.array_equal(got[0, :2], got[0, 2:4])


# ---- 5. layout ---------------------------------------------------------------------------------------------------------------------------
def test_interleaved_strays_and_permutation(seg):
    rng = np.random.default_rng(11)
    T, per = 5, 13
    tr = np.tile(np.arange(T, dtype=np.int32), per)                     # interleaved row by row: 0 1 2 3 4 0 1 ...
    tr = np.insert(tr, [0, 7, 7, 30, len(tr)], -1)                      # rows of no tracklet, at both ends too
    crops = rng.integers(0, 256, (len(tr), 9, 8, 3), dtype=np.uint8)
    crops[tr == -1] = 255                                               # would show in a median if they were counted
    want, want_rows = R.medians(crops, tr, T)
    got, rows, guard = device_call(seg, crops, tr, T)
    assert guard and np.array_equal(rows, want_rows) and np.array_equal(got, want)
    again = device_call(seg, crops, tr, T)
    assert again[0].tobytes() == got.tobytes() and again[1].tobytes() == rows.tobytes()
    p = rng.permutation(len(tr))
    shuffled = device_call(seg, crops[p], tr[p], T)
    assert shuffled[0].tobytes() == got.tobytes() and shuffled[1].tobytes() == rows.tobytes()


def test_70000_tracklets_of_one_image(seg):
    rng = np.random.default_rng(12)
    T = 70000
    crops = rng.integers(0, 256, (T, 8, 8, 1), dtype=np.uint8)
    tr = rng.permutation(T).astype(np.int32)
    got, rows, guard = device_call(seg, crops, tr, T)
    assert guard and (rows == 1).all()
    inverse = np.empty(T, np.int64)
    inverse[tr] = np.arange(T)
    assert np.array_equal(got, crops[inverse, :, :, 0])                 # one image: addImage leaves the image itself (sorted[0])
    some = np.array([0, 1, 65534, 65535, 65536, 69999])                 # ... and the restatement says so where a grid dimension would end
    want, _ = R.medians(crops[inverse[some]], np.arange(len(some)), len(some))
    assert np.array_equal(got[some], want)


def test_one_tracklet_holds_all_rows(seg):
    rng = np.random.default_rng(13)
    crops = rng.integers(0, 256, (1000, 8, 9, 1), dtype=np.uint8)
    tr = np.full(1000, 2, np.int32)
    want, _ = R.medians(crops, tr, 4, incremental=False)
    got, rows, guard = device_call(seg, crops, tr, 4)
    assert rows.tolist() == [0, 0, 1000, 0] and guard and np.array_equal(got, want)


# ---- 6. refusals: nothing is written -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [3, -2])
def test_an_id_outside_the_range_is_invalid(seg, bad):
    crops = np.zeros((6, 8, 8, 1), np.uint8)
    err = refused(seg, crops, [0, 1, 2, bad, 0, -1], 3)
    assert err.code == E_INVALID and "tracklet id" in str(err)


def test_32768_rows_in_one_tracklet_are_unsupported(seg):
    n = R.MAX_ROWS + 1
    crops = np.zeros((n + 2, 8, 8, 1), np.uint8)
    tr = np.full(n + 2, 1, np.int32)
    tr[[5, 100]] = [0, 2]
    err = refused(seg, crops, tr, 3)
    assert err.code == E_UNSUPPORTED and "tracklet 1 " in str(err) and "32768" in str(err)


@pytest.mark.parametrize("W,H,C", [(8, 8, 2), (7, 8, 1), (8, 257, 1), (8, 8, 4), (257, 8, 3), (8, 7, 1)])
def test_sizes_outside_the_range_are_unsupported(seg, W, H, C):
    crops = np.zeros((2, 8, 8, 1), np.uint8)
    err = refused(seg, crops, [0, 0], 1, shape=(H, W, C))
    assert err.code == E_UNSUPPORTED


def test_no_rows_is_ok_and_zeroes_the_outputs(seg):
    got, rows, guard = device_call(seg, np.zeros((0, 11, 13, 3), np.uint8), np.zeros(0, np.int32), 3, off=1)
    assert guard and not got.any() and rows.tolist() == [0, 0, 0]


def test_binding_returns_host_arrays(seg):
    rng = np.random.default_rng(14)
    crops = rng.integers(0, 256, (9, 8, 8, 3), dtype=np.uint8)
    tr = np.array([0, 1, 0, 1, 0, -1, 1, 0, 1], np.int32)
    d_crops, d_tr = torch.from_numpy(crops).cuda(), torch.from_numpy(tr).cuda()
    med, rows = seg.tracklet_medians(d_crops.data_ptr(), 9, 8, 8, 3, d_tr.data_ptr(), 2)
    want, want_rows = R.medians(crops, tr, 2)
    assert med.dtype == np.uint8 and rows.dtype == np.uint32 and np.array_equal(med, want) and np.array_equal(rows, want_rows)
    with pytest.raises(capi.TrexHipError) as e:
        seg.tracklet_medians(d_crops.data_ptr(), 9, 8, 8, 2, d_tr.data_ptr(), 2)
    assert e.value.code == E_UNSUPPORTED


# ---- 7. on the real producer: a pool written by trexhip_crops_device goes straight into the call -----------------------------------------
def test_pool_of_crops_device_without_a_host_copy():
    fr, bg = synth.batch("C2", 2)
    n, H, W = fr.shape
    s = capi.Segmenter(capi.default_params(W, H, max_batch=n))
    try:
        s.set_background(bg)
        d = torch.from_numpy(fr).cuda()
        s.segment_device(d.data_ptr(), n)
        res = s.fetch()
        nb = sum(len(r.blobs) for r in res)
        assert nb >= 4
        pool = torch.zeros((nb, 80, 80), dtype=torch.uint8, device="cuda")
        s.crops_device(pool.data_ptr(), nb)
        T = 3
        tr = (np.arange(nb) % (T + 1) - 1).astype(np.int32)             # -1 0 1 2 -1 0 ...: every blob of the batch, one in four to no tracklet
        d_tr = torch.from_numpy(tr).cuda()
        med, rows = s.tracklet_medians(pool.data_ptr(), nb, 80, 80, 1, d_tr.data_ptr(), T)
        crops = pool.cpu().numpy()
        assert crops.any()
        want, want_rows = R.medians(crops[..., None], tr, T)
        assert np.array_equal(rows, want_rows) and np.array_equal(med, want) and med.any()
    finally:
        s.close()
