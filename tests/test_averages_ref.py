"""tests/averages_ref.py (the restatement of VINetwork::paverages and of check_additional_range's arg-max scan that the GPU tests of
trexhip_class_averages_device are held against), pinned two ways: a case worked out by hand in which the order of the additions shows in
the bits, and random inputs against a float64 mean."""
import numpy as np

import averages_ref as A

F = np.float32
E = F(2.0 ** -24)          # half an ulp of 1.0f: 1 + E rounds back to 1 (ties to even), E + E = 2^-23 is one ulp of 1


def test_the_sum_is_sequential_in_row_order():
    # id 7 owns rows 0, 2, 3 (class 0: 1, E, E) and id 3 rows 1, 4, 5 (class 0: E, E, 1), interleaved.
    # id 7: (1 + E) + E = 1 + E = 1: stays exactly 1.0.  A pairwise or reordered sum, 1 + (E + E), would give 1 + 2^-23.
    # id 3: (E + E) + 1 = 1 + 2^-23.
    # class 1 is 3.0 in every row: sum 9, mean 3 exactly.
    probs = np.array([[1, 3], [E, 3], [E, 3], [E, 3], [E, 3], [1, 3]], F)
    ids = [7, 3, 7, 7, 3, 3]
    av = A.paverages(probs, ids)
    assert list(av) == [3, 7]
    s7, v7 = av[7]
    s3, v3 = av[3]
    assert s7 == F(3) and s3 == F(3) and s7.dtype == F and v7.dtype == F
    one_up = F(1) + F(2.0 ** -23)
    assert v7[0] == F(1) / F(3) and v7[0] != one_up / F(3)
    assert v3[0] == one_up / F(3) and v3[0] != F(1) / F(3)
    assert v7[1] == F(3) and v3[1] == F(3)


def test_the_division_is_one_float32_division():
    # 0.1f + 0.2f + 0.3f in float32, then / 3.0f: not the float64 mean rounded
    probs = np.array([[0.1], [0.2], [0.3]], F)
    s, v = A.paverages(probs, [0, 0, 0])[0]
    want = F(F(F(F(0) + F(0.1)) + F(0.2)) + F(0.3)) / F(3)
    assert v[0].tobytes() == want.tobytes()


def test_argmax_scan():
    assert A.argmax_scan(np.array([0.2, 0.5, 0.5, 0.1], F)) == (1, F(0.5))                    # the first index wins a tie
    assert A.argmax_scan(np.zeros(4, F)) == (-1, F(0))                                          # nothing above 0
    assert A.argmax_scan(np.array([-1, -0.0, 0], F)) == (-1, F(0))
    with np.errstate(invalid="ignore"):
        assert A.argmax_scan(np.array([np.nan, np.nan], F)) == (-1, F(0))                       # a NaN is never taken
        assert A.argmax_scan(np.array([np.nan, 0.25, np.nan, 0.25], F)) == (1, F(0.25))
    assert A.argmax_scan(np.array([0, 0, 1e-45], F)) == (2, F(1e-45))


def test_class_averages_dense_outputs():
    # keys 0 and 2 have rows, key 1 none; key 2's row is NaN in class 1; key 0 averages to a tie
    probs = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.125, np.nan, 0.0]], F)
    samples, values, max_index, max_p = A.class_averages(probs, [0, 0, 2], 3)
    assert samples.tolist() == [2.0, 0.0, 1.0]
    assert values[0].tolist() == [0.375, 0.375, 0.25] and values[1].tolist() == [0, 0, 0]
    assert max_index.tolist() == [0, -1, 0] and max_p.tolist() == [0.375, 0.0, 0.125]
    assert np.isnan(values[2][1])


def test_random_inputs_against_a_float64_mean():
    # a float32 sum of m non-negative terms is within (m - 1) * 2^-24 relative of the exact sum, the division adds half an ulp: m * 2^-24
    rng = np.random.default_rng(3)
    for n, classes, n_ids in [(1, 1, 1), (257, 7, 3), (3000, 100, 10)]:
        probs = rng.random((n, classes)).astype(F) ** 4
        probs = (probs / probs.sum(axis=1, keepdims=True)).astype(F)
        ids = rng.integers(0, n_ids, n)
        av = A.paverages(probs, ids)
        assert sorted(av) == sorted(set(ids.tolist()))
        for k, (s, v) in av.items():
            rows = probs[ids == k].astype(np.float64)
            m = len(rows)
            assert s == F(m)
            mean = rows.mean(axis=0)
            assert (np.abs(v.astype(np.float64) - mean) <= m * 2.0 ** -24 * mean).all()
