"""Line-by-line NumPy restatement of the two end-of-epoch validation reductions of the reference (a plain module, not a test):

  calculate_uniqueness   Accumulation::calculate_uniqueness, Application/src/tracker/ui/Accumulation.cpp:767-879
  per_class_accuracy     ValidationCallback.plot_comparison_raw's column 3, Application/src/tracker/python/visual_recognition_torch.py:406-451
  confusion              confusion[target][np.argmax(row)] += 1, whose diagonal over its row sums is that column

with the reference's number types: float32 where it computes in float, Python floats (float64) where it computes in double.  One thing is
fixed that the reference leaves open: accum_p (:826-832) is summed over a frame's identities in ASCENDING IDENTITY ORDER (the reference
iterates a hash_map, so its order is unspecified); `order` overrides it, to measure what that choice costs.
"""
import math
import numpy as np

F = np.float32
# static const float NORMAL = (1+expf(-1*float(M_PI)*1));   (:835)   expf of glibc is correctly rounded here: the double exp, rounded once
NORMAL = F(1) + F(math.exp(float(F(-1) * F(math.pi) * F(1))))


def logic_regression(x):
    """:834-838  1/(1+exp(-x*M_PI*1))*NORMAL -- x float, M_PI double: evaluated in double"""
    return 1.0 / (1.0 + math.exp(-float(F(x)) * math.pi * 1)) * float(NORMAL)


def row_identity(row):
    """:804-814 -> (max_id or None, max_p)"""
    max_id, max_p = None, F(0)
    for i, p in enumerate(row):
        if p > max_p:                   # false for NaN
            max_p, max_id = p, i
    return max_id, max_p


def rows_identity(pred):
    """row_identity for every row at once -> (ids int64 [n], -1 = none; max_p float32 [n]).  The scan takes the first index of the largest
    entry that is > 0: np.argmax (first maximum) over the row with everything that is not > 0 (NaN included) set to 0."""
    pred = np.ascontiguousarray(pred, F)
    if pred.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, F)
    with np.errstate(invalid="ignore"):
        pos = np.where(pred > 0, pred, F(0))
    ids = pos.argmax(axis=1)
    max_p = pos[np.arange(len(pos)), ids]
    return np.where(max_p > 0, ids, -1), max_p


def calculate_uniqueness(predictions, frame_ranges, order=None):
    """predictions float32 [n][N]; frame_ranges [(start, end)] in the order of the reference's std::map (ascending frames).
    order(ids) -> the order accum_p is summed in (default: ascending).  Returns a dict with the names of trexhip_uniqueness_result and
    of the call's arrays; the doubles the reference forms (:878, :875) are cast to float32 where it casts them."""
    pred = np.ascontiguousarray(predictions, F)
    N = pred.shape[1]
    row_ids, row_max = rows_identity(pred)
    row_ids = row_ids.tolist()
    good_frames = bad_frames = 0
    percentages = rpercentages = 0.0
    unique_percent, unique_percent_raw = [], []
    per_identity = np.zeros(N, F)               # unique_percent_per_identity
    per_identity_samples = np.zeros(N, F)
    frames_seen = np.zeros(N, np.int64)
    for start, end in frame_ranges:
        probs = {}                              # its keys are unique_ids
        for i in range(start, end):
            max_id, max_p = row_ids[i], row_max[i]              # = row_identity(pred[i]), tests/test_uniqueness_ref.py
            if max_id >= 0:
                probs[max_id] = max(probs.get(max_id, F(0)), max_p)
        length = end - start
        p = 0.0 if length <= 0 else float(F(len(probs)) / F(length))        # size / float(length), kept in a double
        accum_p = F(0)
        ids = sorted(probs) if order is None else order(sorted(probs))
        for k in ids:
            accum_p = F(accum_p + probs[k])
        for k in sorted(probs):
            per_identity[k] = F(per_identity[k] + probs[k])
            per_identity_samples[k] += F(1)
            frames_seen[k] += 1
        unique_percent_raw.append(F(p))
        rpercentages += p
        if probs:
            p = logic_regression(F(accum_p / F(len(probs)))) * p
        unique_percent.append(F(p))
        percentages += p
        if len(probs) == length:
            good_frames += 1
        else:
            bad_frames += 1
    per_class = np.zeros(N, F)
    seen = per_identity_samples > 0
    per_class[seen] = per_identity[seen] / per_identity_samples[seen]
    nf = len(frame_ranges)
    return {"good_frames": good_frames, "bad_frames": bad_frames, "good_ratio": F(F(good_frames) / F(good_frames + bad_frames)),
            "mean_unique": F(percentages / float(nf)), "mean_unique_raw": F(rpercentages / float(nf)),
            "unique_percent": np.array(unique_percent, F), "unique_percent_raw": np.array(unique_percent_raw, F),
            "uniqueness_per_class": per_class, "frames_per_class": frames_seen}


def confusion(predictions, targets, classes):
    """confusion[target][np.argmax(row)] += 1 (np.argmax: first maximum, first NaN if there is one)"""
    conf = np.zeros((classes, classes), np.uint32)
    pred = np.ascontiguousarray(predictions, F).reshape(-1, classes)
    if len(pred):
        np.add.at(conf, (np.asarray(targets, np.int64), pred.argmax(axis=1)), 1)
    return conf


def per_class_accuracy(predictions, targets, classes):
    """plot_comparison_raw's result[:, 3] (:409-449): zeros, and for every class that has images (y.argmax(axis=1) == i).sum() / len(y)"""
    pred = np.ascontiguousarray(predictions, F).reshape(-1, classes)
    targets = np.asarray(targets, np.int64)
    result = np.zeros(classes, float)
    for i in range(classes):
        y = pred[targets == i]
        if len(y) == 0:
            continue
        result[i] = (y.argmax(axis=1) == i).sum() / len(y)
    return result
