"""tests/tracklet_median_ref.py against itself and against an independent reading: the incremental restatement of hist_utils::addImage
(Export.cpp:91-116) ends at final_median, final_median is np.sort(stack, axis=0)[m // 2], and its gray is oracle.bgr2gray."""
import numpy as np
import pytest

import tracklet_median_ref as R
from tracklet_median_cases import constructed
from oracle import oracle

COUNTS = [1, 2, 3, 4, 255, 256, 257]


@pytest.mark.parametrize("m", COUNTS)
def test_incremental_walk_ends_at_final_median_and_at_the_sorted_stack(m):
    rng = np.random.default_rng(100 + m)
    for stack in (constructed(m), rng.integers(0, 256, (m, 3, 5), dtype=np.uint8), rng.integers(96, 104, (m, 3, 5), dtype=np.uint8)):
        st = R.init(*stack.shape[1:])
        assert st["med"].dtype == np.uint8 and not st["med"].any() and st["h"].dtype == np.int16
        for k, img in enumerate(stack):
            med = R.add_image(st, img)
            # after every image, not only the last: the running value is the sorted prefix's [count // 2]
            assert np.array_equal(med, np.sort(stack[:k + 1], axis=0)[(k + 1) // 2])
        want = np.sort(stack, axis=0)[m // 2]
        assert np.array_equal(st["med"], want)
        assert np.array_equal(R.final_median(st["h"], st["count"]), want)
        assert np.array_equal(R.final_median(R.histograms(stack), np.full(stack.shape[1:], m)), want)
        # the order of the images does not matter
        assert np.array_equal(R.tracklet_median(stack[rng.permutation(m)])[0], want)


def test_even_count_takes_the_upper_median():
    stack = np.array([0, 255, 0, 255], np.uint8).reshape(4, 1, 1)
    assert R.tracklet_median(stack)[0][0, 0] == 255
    assert R.tracklet_median(stack[:3])[0][0, 0] == 0
    assert R.tracklet_median(stack[:2])[0][0, 0] == 255
    assert R.tracklet_median(stack[:1])[0][0, 0] == 0


def test_final_median_at_the_count_limit():
    m = R.MAX_ROWS
    hist = np.zeros((4, 256), np.int32)
    hist[0, 9] = m                                                      # one bin holds the maximum a short takes
    hist[1, 3], hist[1, 250] = m // 2, m - m // 2                       # 16383 | 16384: rank 16383 is the first 250
    hist[2, 3], hist[2, 250] = m - m // 2, m // 2                       # 16384 | 16383: rank 16383 is the last 3
    hist[3, 255] = m
    assert R.final_median(hist, np.full(4, m)).tolist() == [9, 250, 3, 255]
    with pytest.raises(AssertionError):
        st = R.init(1, 1)
        st["h"][0, 0, 5], st["count"][0, 0] = m, m
        R.add_image(st, np.full((1, 1), 5, np.uint8))


def test_a_tracklet_without_rows_keeps_the_image_init_leaves():
    crops = np.full((3, 8, 8, 1), 9, np.uint8)
    med, rows = R.medians(crops, [2, -1, 2], 3)
    assert rows.tolist() == [0, 0, 2] and not med[:2].any() and (med[2] == 9).all()
    assert np.array_equal(R.medians(crops, [2, -1, 2], 3, incremental=False)[0], med)


def test_gray_is_the_oracles():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 41, 3), dtype=np.uint8)
    img[0, :4] = [[255, 255, 255], [0, 0, 0], [255, 0, 255], [0, 255, 0]]
    assert np.array_equal(R.bgr2gray(img), oracle.bgr2gray(img))
    assert np.array_equal(R.to_gray(img), oracle.bgr2gray(img))
    one = img[..., :1]
    assert np.array_equal(R.to_gray(one), one[..., 0]) and np.array_equal(R.to_gray(one[..., 0]), one[..., 0])
    with pytest.raises(ValueError):
        R.to_gray(img[..., :2])


def test_medians_of_colour_crops_go_through_the_gray():
    rng = np.random.default_rng(6)
    crops = rng.integers(0, 256, (7, 8, 9, 3), dtype=np.uint8)
    tr = np.array([0, 1, 0, -1, 1, 0, 1])
    med, rows = R.medians(crops, tr, 2)
    gray = oracle.bgr2gray(crops.reshape(-1, 3)).reshape(7, 8, 9)
    assert rows.tolist() == [3, 3]
    for t in range(2):
        assert np.array_equal(med[t], np.sort(gray[tr == t], axis=0)[3 // 2])
