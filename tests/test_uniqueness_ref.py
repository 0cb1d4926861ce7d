"""tests/uniqueness_ref.py (the restatement of Accumulation::calculate_uniqueness and of plot_comparison_raw's column 3 that the GPU
tests of trexhip_validation_metrics_device are held against) on frames worked out by hand here."""
import ctypes
import ctypes.util
import math
import numpy as np
import pytest
import uniqueness_ref as U

F = np.float32


def one_hot(ids, classes, p=1.0):
    out = np.zeros((len(ids), classes), F)
    out[np.arange(len(ids)), ids] = p
    return out


def test_normal_is_the_c_expression():
    # static const float NORMAL = (1+expf(-1*float(M_PI)*1)) with the C library's expf
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    assert U.NORMAL == F(1) + F(libm.expf(F(-1) * F(math.pi)))
    assert U.NORMAL.dtype == F and abs(float(U.NORMAL) - (1 + math.exp(-math.pi))) < 1e-7


def test_two_samples_with_the_same_identity_make_a_bad_frame():
    r = U.calculate_uniqueness(one_hot([0, 0], 4, 0.75), [(0, 2)])
    assert r["unique_percent_raw"][0] == F(0.5) and (r["good_frames"], r["bad_frames"]) == (0, 1)
    # one identity, accum_p = 0.75: logistic(0.75 / 1) * 0.5
    want = 1.0 / (1.0 + math.exp(-0.75 * math.pi)) * float(U.NORMAL) * 0.5
    assert r["unique_percent"][0] == F(want)
    assert r["good_ratio"] == 0 and r["mean_unique"] == F(want) and r["mean_unique_raw"] == F(0.5)
    assert r["uniqueness_per_class"].tolist() == [0.75, 0, 0, 0]


def test_all_distinct_with_probability_one_is_exactly_one():
    r = U.calculate_uniqueness(one_hot([2, 0, 3, 1], 4), [(0, 4)])
    assert r["unique_percent_raw"][0] == 1 and r["unique_percent"][0] == 1 and (r["good_frames"], r["bad_frames"]) == (1, 0)
    assert r["good_ratio"] == 1 and r["mean_unique"] == 1
    # in double the logistic of 1 is a little above 1 (that is what NORMAL is for): only the cast to float makes it 1
    assert 1.0 < U.logic_regression(1.0) < 1.0 + 2.0 ** -24


def test_an_empty_range_is_zero_and_good():
    r = U.calculate_uniqueness(one_hot([0, 1], 2), [(1, 1), (0, 2)])
    assert r["unique_percent"][0] == 0 and r["unique_percent_raw"][0] == 0 and (r["good_frames"], r["bad_frames"]) == (2, 0)
    assert r["mean_unique"] == F(0.5) and r["mean_unique_raw"] == F(0.5)


def test_rows_without_a_positive_entry_have_no_identity():
    rows = np.zeros((4, 3), F)
    rows[1] = np.nan
    rows[2] = [-1, -2, -0.5]
    rows[3] = [np.nan, 0.25, 0.0]                 # a NaN beside a positive entry: the positive entry is the identity
    for k in range(3):
        assert U.row_identity(rows[k])[0] is None
    assert U.row_identity(rows[3]) == (1, F(0.25))
    ids, max_p = U.rows_identity(rows)
    assert ids.tolist() == [-1, -1, -1, 1] and max_p.tolist() == [0, 0, 0, 0.25]
    r = U.calculate_uniqueness(rows, [(0, 3), (0, 4)])
    assert r["unique_percent"].tolist()[0] == 0 and r["unique_percent_raw"].tolist() == [0, 0.25] and r["bad_frames"] == 2
    # np.argmax, which the confusion matrix counts by: the first NaN, else the first maximum
    assert U.confusion(rows, [0, 0, 2, 1], 3).tolist() == [[2, 0, 0], [1, 0, 0], [0, 0, 1]]
    assert U.per_class_accuracy(rows, [0, 0, 2, 1], 3).tolist() == [1.0, 0.0, 1.0]


def test_a_tie_goes_to_the_lower_index():
    rows = np.array([[0.5, 0.5, 0.0], [0.1, 0.45, 0.45]], F)
    assert U.row_identity(rows[0]) == (0, F(0.5)) and U.row_identity(rows[1]) == (1, F(0.45))
    assert U.rows_identity(rows)[0].tolist() == [0, 1]
    assert U.confusion(rows, [1, 1], 3).tolist() == [[0, 0, 0], [1, 1, 0], [0, 0, 0]]


def test_vector_and_scalar_row_scan_agree():
    rng = np.random.default_rng(3)
    rows = rng.random((200, 7)).astype(F)
    rows[rng.random(rows.shape) < 0.2] = 0
    rows[rng.random(rows.shape) < 0.05] = np.nan
    rows[rng.random(rows.shape) < 0.05] *= -1
    rows[:20, 3] = rows[:20, 5] = 2.0             # ties of the maximum
    rows[20:25] = np.float32(1e-45) * (rows[20:25] > 0.5)        # denormal maxima
    ids, max_p = U.rows_identity(rows)
    for k, row in enumerate(rows):
        i, p = U.row_identity(row)
        assert (i if i is not None else -1) == ids[k] and p == max_p[k]


def test_per_class_accuracy_leaves_empty_classes_at_zero():
    rows = one_hot([0, 0, 1, 3], 4)
    acc = U.per_class_accuracy(rows, [0, 1, 1, 3], 4)
    assert acc.tolist() == [1.0, 0.5, 0.0, 1.0] and not np.isnan(acc).any()
    conf = U.confusion(rows, [0, 1, 1, 3], 4)
    assert conf.sum() == 4 and np.diagonal(conf).tolist() == [1, 1, 0, 1]


@pytest.mark.parametrize("classes", [3, 16, 100, 1024])
def test_what_fixing_the_summation_order_costs(classes):
    # the reference sums accum_p in its hash_map's order; any order moves the float32 sum of `classes` values in [0, 1] by at most
    # classes * 2^-24 relative (each of the classes - 1 additions rounds by at most 2^-24 of a partial sum that is at most the total),
    # and the logistic's slope times its argument is below 1, so unique_percent moves by no more
    rng = np.random.default_rng(classes)
    rows = one_hot(np.arange(classes), classes)
    rows[np.arange(classes), np.arange(classes)] = rng.random(classes).astype(F) * 0.9 + 0.1
    base = U.calculate_uniqueness(rows, [(0, classes)])["unique_percent"][0]
    worst = 0.0
    for k in range(100):
        perm = np.random.default_rng([classes, k])
        got = U.calculate_uniqueness(rows, [(0, classes)], order=lambda ids: list(perm.permutation(ids)))["unique_percent"][0]
        worst = max(worst, abs(float(got) - float(base)) / float(base))
    assert worst <= classes * 2.0 ** -24, worst
