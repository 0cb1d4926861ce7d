"""NumPy restatement of VINetwork::paverages (Application/src/tracker/ml/VisualIdentification.h:145-180) and of the arg-max scan of
Accumulation::check_additional_range (Application/src/tracker/ui/Accumulation.cpp:526-541), line by line: what
trexhip_class_averages_device is held against bit for bit.  Every addition is an explicit np.float32 operation in row order."""
import numpy as np

F = np.float32


def paverages(probs, ids):
    """probs float32 [n][classes], ids [n] (any hashable, ordered keys) -> {id: (samples float32, values float32 [classes])} in key order.
    values[c] = ((0 + p[i0][c]) + p[i1][c]) + ... over the id's rows in ascending row order (:159-175), each sum rounded to float32, then
    one float32 division by samples (:177-178)."""
    probs = np.asarray(probs, F)
    sums, samples = {}, {}
    with np.errstate(invalid="ignore", over="ignore"):
        for i, k in enumerate(ids):
            k = int(k)
            if k not in sums:                                  # values.resize(N); samples = 0   (:166-169)
                sums[k] = np.zeros(probs.shape[1], F)
                samples[k] = F(0)
            samples[k] = F(samples[k] + F(1))                  # ++samples   (:171)
            sums[k] = (sums[k] + probs[i]).astype(F)           # std::transform(..., std::plus<>{})   (:174): float32 + float32, element by element
        return {k: (samples[k], (sums[k] / samples[k]).astype(F)) for k in sorted(sums)}


def argmax_scan(values):
    """(:526-541): max_index = -1, max_p = 0; take i iff v > max_p -> (max_index, max_p).  The first index wins a tie, a NaN is never taken
    (NaN > x is false), a row with nothing above 0 gives (-1, 0)."""
    max_index, max_p = -1, F(0)
    for i, v in enumerate(np.asarray(values, F)):
        if v > max_p:
            max_index, max_p = i, v
    return max_index, max_p


def class_averages(probs, keys, n_ids):
    """what trexhip_class_averages_device returns for dense keys 0..n_ids-1: (samples [n_ids], values [n_ids][classes], max_index [n_ids],
    max_p [n_ids]); a key without rows has samples 0, all-zero values (no division), max_index -1, max_p 0"""
    probs = np.asarray(probs, F)
    av = paverages(probs, keys)
    samples, values = np.zeros(n_ids, F), np.zeros((n_ids, probs.shape[1]), F)
    max_index, max_p = np.full(n_ids, -1, np.int32), np.zeros(n_ids, F)
    for k, (s, v) in av.items():
        samples[k], values[k] = s, v
    with np.errstate(invalid="ignore"):
        for k in range(n_ids):
            max_index[k], max_p[k] = argmax_scan(values[k])
    return samples, values, max_index, max_p
