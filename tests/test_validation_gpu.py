"""End-of-epoch validation of identity training on the device: trexhip_train_predict_device (softmax rows from the trainer's current
weights), trexhip_validation_metrics_device (confusion matrix + Accumulation::calculate_uniqueness) and train_loop.ResidentValidation,
against tests/uniqueness_ref.py (the line-by-line restatement) and the float64 network restatement."""
import ctypes as C
import numpy as np
import pytest
import torch

import identity_synth
import uniqueness_ref as U
from oracle import cnn_oracle
from trex_amd import capi, train_loop, weights

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID = -1


@pytest.fixture(scope="module")
def seg():
    p = capi.default_params(64, 64)
    p.max_batch = 1
    s = capi.Segmenter(p)
    yield s
    s.close()


# ---- 1. the metrics on injected probabilities -------------------------------------------------------------------------------------------
CLASSES = [2, 3, 63, 64, 65, 100, 129, 256, 1024]
N_FRAMES = [1, 2, 257, 1000]
MAX_ROWS = 5000


def special_rows(classes, rng):
    """all-zero, all-negative, one NaN, ties of the maximum at (0, 1) and (classes - 2, classes - 1), a maximum of exactly 1.0f, denormal maxima"""
    def soft():
        r = rng.random(classes).astype(F) ** 8
        return (r / r.sum() * F(0.5)).astype(F)
    rows = [np.zeros(classes, F), -soft() - F(0.01)]
    r = soft(); r[rng.integers(classes)] = np.nan; rows.append(r)
    r = soft(); r[0] = r[1] = F(0.75); rows.append(r)
    r = soft(); r[classes - 2] = r[classes - 1] = F(0.75); rows.append(r)
    r = np.zeros(classes, F); r[rng.integers(classes)] = F(1.0); rows.append(r)
    r = np.zeros(classes, F); r[classes - 1] = F(1e-45); r[0] = F(3e-45) if classes > 2 else F(1e-45); rows.append(r)
    r = np.full(classes, F(1e-45), F); rows.append(r)                       # a tie of denormals over the whole row
    return np.stack(rows)


def make_case(classes, n_frames):
    rng = np.random.default_rng([classes, n_frames])
    lens = [300, classes + 1, 0, 1, 70, classes, 2, classes - 1]
    lengths = [lens[k] if k < 8 else int(rng.choice(lens)) for k in range(n_frames)]
    gaps = [int(g) for g in rng.integers(0, 3, n_frames)]
    n = min(sum(lengths) + sum(gaps) + 3, MAX_ROWS)
    n = max(n, max(lengths) + 3, 16)
    ranges, cursor, lim = [], 0, n - 3                       # the last three rows belong to no frame
    for ln, g in zip(lengths, gaps):
        if cursor + ln > lim:                                # the pool of rows is used up: go round (later frames overlap earlier ones)
            cursor = int(rng.integers(0, lim - ln + 1))
        ranges.append((cursor, cursor + ln))
        cursor += ln + g                                     # g > 0 leaves a gap
    if n_frames >= 2:                                        # two ranges overlap, whatever the draw
        a, b = ranges[0]
        ln = lengths[1]
        s = max(0, min(b - 1, lim - ln))
        ranges[1] = (s, s + ln)
    rows = rng.random((n, classes)).astype(F) ** 8
    rows = (rows / rows.sum(axis=1, keepdims=True)).astype(F)
    sp = special_rows(classes, rng)
    rows[:len(sp)] = sp                                      # frame 0 starts at row 0
    at = rng.choice(np.arange(len(sp), n), size=min(4 * len(sp), n - len(sp)), replace=False)
    rows[at] = sp[np.arange(len(at)) % len(sp)]              # ... and scattered through the other frames
    targets = rng.integers(0, classes, n).astype(np.int32)
    return rows, targets, np.array(ranges, np.int32)


def as_bytes(m):
    parts = [m.confusion, m.unique_percent, m.unique_percent_raw, m.uniqueness_per_class,
             np.array([m.good_frames, m.bad_frames], np.int64), np.array([m.good_ratio, m.mean_unique, m.mean_unique_raw], np.float64)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def held_to_the_bars(m, want, classes):
    """the bars of the uniqueness outputs: trexhip_validation_metrics_device against tests/uniqueness_ref.py"""
    assert (m.good_frames, m.bad_frames) == (want["good_frames"], want["bad_frames"])
    # the set of identities per frame: a ratio of two small integers in float32, bit for bit
    assert m.unique_percent_raw.tobytes() == want["unique_percent_raw"].tobytes()
    # the double exp is the one operation that libm and the device may round differently (1 ulp of a double), then one rounding to float
    d = np.abs(m.unique_percent.astype(np.float64) - want["unique_percent"].astype(np.float64))
    print(f"classes {classes}: max |unique_percent - ref| = {d.max():.3g}")
    assert d.max() <= 2.4e-7, d.max()
    for k in ("good_ratio", "mean_unique", "mean_unique_raw"):
        w = want[k]
        assert abs(float(F(getattr(m, k))) - float(w)) <= float(np.spacing(F(abs(w)))), (k, getattr(m, k), w)
    bound = want["frames_per_class"] * 2.0 ** -24 * want["uniqueness_per_class"].astype(np.float64)
    assert (np.abs(m.uniqueness_per_class.astype(np.float64) - want["uniqueness_per_class"]) <= bound).all()


@pytest.mark.parametrize("n_frames", N_FRAMES)
@pytest.mark.parametrize("classes", CLASSES)
def test_metrics_on_injected_probabilities(seg, classes, n_frames):
    rows, targets, ranges = make_case(classes, n_frames)
    n = len(rows)
    covered = np.zeros(n + 1, np.int64)
    for a, b in ranges:
        covered[a] += 1; covered[b] -= 1
    covered = np.cumsum(covered)[:n]
    if n_frames >= 2:
        assert (covered > 1).any()
    assert (covered == 0).any(), "the ranges must leave a gap"
    d_rows = torch.from_numpy(rows).cuda()
    d_targets = torch.from_numpy(targets).cuda()
    m = seg.validation_metrics(d_rows.data_ptr(), n, classes, d_targets_ptr=d_targets.data_ptr(), frame_ranges=ranges)
    again = seg.validation_metrics(d_rows.data_ptr(), n, classes, d_targets_ptr=d_targets.data_ptr(), frame_ranges=ranges)
    assert as_bytes(m) == as_bytes(again), "two runs differ"
    with np.errstate(invalid="ignore"):
        want = U.calculate_uniqueness(rows, [tuple(int(v) for v in r) for r in ranges])
        conf = U.confusion(rows, targets, classes)
        acc = U.per_class_accuracy(rows, targets, classes)
    assert np.array_equal(m.confusion, conf)
    assert np.array_equal(m.per_class_accuracy, acc) and not np.isnan(m.per_class_accuracy).any()
    held_to_the_bars(m, want, classes)
    # each half alone gives the same
    only_conf = seg.validation_metrics(d_rows.data_ptr(), n, classes, d_targets_ptr=d_targets.data_ptr())
    only_uniq = seg.validation_metrics(d_rows.data_ptr(), n, classes, frame_ranges=ranges)
    assert np.array_equal(only_conf.confusion, conf) and only_conf.unique_percent is None
    assert only_uniq.confusion is None and only_uniq.unique_percent.tobytes() == m.unique_percent.tobytes() and only_uniq.mean_unique == m.mean_unique


def test_an_unaligned_row_base_takes_the_scalar_path(seg):
    classes = 64
    rows, targets, ranges = make_case(classes, 2)
    n = len(rows)
    buf = torch.zeros(n * classes + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(rows.reshape(-1)).cuda()
    d_targets = torch.from_numpy(targets).cuda()
    m = seg.validation_metrics(buf.data_ptr() + 4, n, classes, d_targets_ptr=d_targets.data_ptr(), frame_ranges=ranges)
    aligned = torch.from_numpy(rows).cuda()
    ref = seg.validation_metrics(aligned.data_ptr(), n, classes, d_targets_ptr=d_targets.data_ptr(), frame_ranges=ranges)
    assert as_bytes(m) == as_bytes(ref)


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------
def raw_call(seg, d_rows, n, classes, d_targets, ranges, n_frames):
    """the C call with sentinel-filled outputs -> (return code, outputs untouched?)"""
    conf = np.full((max(classes, 1), max(classes, 1)), 0xABABABAB, np.uint32)
    res = capi.UniquenessResult(7, 7, -7.0, -7.0, -7.0)
    nf = max(n_frames, 1)
    up, upr, upc = np.full(nf, -7, F), np.full(nf, -7, F), np.full(max(classes, 1), -7, F)
    fr = np.ascontiguousarray(ranges, np.int32) if ranges is not None else None
    rc = capi.lib().trexhip_validation_metrics_device(seg.handle, C.c_void_p(d_rows), n, classes, C.c_void_p(d_targets), fr.ctypes.data_as(C.c_void_p) if fr is not None else None,
                                                      n_frames, conf.ctypes.data_as(C.c_void_p), C.byref(res), up.ctypes.data_as(C.c_void_p),
                                                      upr.ctypes.data_as(C.c_void_p), upc.ctypes.data_as(C.c_void_p))
    untouched = ((conf == 0xABABABAB).all() and (up == -7).all() and (upr == -7).all() and (upc == -7).all()
                 and (res.good_frames, res.bad_frames, res.good_ratio, res.mean_unique, res.mean_unique_raw) == (7, 7, -7.0, -7.0, -7.0))
    return rc, untouched


def test_refusals(seg):
    classes, n = 5, 12
    rng = np.random.default_rng(1)
    rows = torch.from_numpy(rng.random((n, classes)).astype(F)).cuda()
    targets = torch.from_numpy(rng.integers(0, classes, n).astype(np.int32)).cuda()
    ok = [(0, 4), (4, 12)]
    assert raw_call(seg, rows.data_ptr(), n, classes, targets.data_ptr(), ok, 2) == (0, False)
    cases = {"end > n": ([(0, 4), (4, 13)], 2, classes), "start > end": ([(5, 4), (4, 12)], 2, classes), "negative start": ([(-1, 4), (4, 12)], 2, classes),
             "n_frames = 0 with ranges": (ok, 0, classes), "classes = 0": (ok, 2, 0), "classes = 1025": (ok, 2, 1025)}
    for name, (ranges, nf, cl) in cases.items():
        rc, untouched = raw_call(seg, rows.data_ptr(), n, cl, targets.data_ptr(), ranges, nf)
        assert rc == E_INVALID and untouched, name
        assert b"trexhip_validation_metrics_device" in capi.lib().trexhip_last_error()
    bad = targets.clone()
    bad[7] = classes
    rc, untouched = raw_call(seg, rows.data_ptr(), n, classes, bad.data_ptr(), ok, 2)          # flagged by the device
    assert rc == E_INVALID and untouched
    with pytest.raises(capi.TrexHipError):
        seg.validation_metrics(rows.data_ptr(), n, classes, d_targets_ptr=bad.data_ptr())
    # and the context goes on
    assert raw_call(seg, rows.data_ptr(), n, classes, targets.data_ptr(), ok, 2) == (0, False)


# ---- 3. predict_device ------------------------------------------------------------------------------------------------------------------
P_CLASSES, MAX_BATCH = 16, 8


def synth(ids, labels, seed, ch, u8):
    x = ids.render(labels, seed)
    if ch == 3:
        x = x * np.array([1.0, 0.8, 0.6], F)
    return np.rint(x).astype(np.uint8) if u8 else np.ascontiguousarray(x, F)


def make_trainer(seg, ch, precision):
    """the trainer of cases 3 and 4: synthetic weights, then two steps on a batch of identity_synth so that the weights are the trainer's own"""
    ids = identity_synth.Identities(P_CLASSES, seed=5)
    tr = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(P_CLASSES, 21 + ch, channels=ch), P_CLASSES, ch), max_batch=MAX_BATCH, lr=1e-3, seed=9,
                      precision=precision)
    y = ids._labels(MAX_BATCH, 1)
    x = synth(ids, y, 1, ch, False)
    for _ in range(2):
        tr.step(x, y)
    return ids, tr


@pytest.fixture(scope="module", params=[(1, 0), (1, 1), (3, 0), (3, 1)], ids=lambda p: f"ch{p[0]}-precision{p[1]}")
def trained(seg, request):
    ch, precision = request.param
    ids, tr = make_trainer(seg, ch, precision)
    y = ids._labels(21, 2)
    crops = synth(ids, y, 2, ch, True)
    state = weights.unpack_blob(tr.export())[0]
    want = cnn_oracle.predict(state, crops, threads=8, dtype=torch.float64)[0]          # computed once, shared, never changed
    yield {"ids": ids, "tr": tr, "ch": ch, "precision": precision, "crops": crops, "y": y, "want": want}
    tr.close()


def predict(tr, crops, n=None):
    n = len(crops) if n is None else n
    d = torch.from_numpy(crops).cuda()
    out = torch.full((n, P_CLASSES), -1.0, dtype=torch.float32, device="cuda")
    tr.predict_device(d.data_ptr(), n, out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 21])
def test_predict_rows_equal_the_float64_network(trained, n):
    # measured on an MI355X: max |p - p_float64| = 7.1e-7 over 1 and 3 channels, both precisions and every n (bar 1e-4)
    rows = predict(trained["tr"], trained["crops"][:n])
    err = float(np.abs(rows - trained["want"][:n]).max())
    print(f"predict_device ch {trained['ch']} precision {trained['precision']} n {n}: max |dp| = {err:.3g}")
    assert err <= 1e-4, f"max |p - p_float64| = {err}"
    assert np.abs(rows.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6


def test_a_row_does_not_depend_on_its_chunk(trained):
    tr, crops = trained["tr"], trained["crops"]
    whole = predict(tr, crops)
    parts = np.concatenate([predict(tr, crops[k:k + 7]) for k in (0, 7, 14)])
    assert whole.tobytes() == parts.tobytes()


def test_argmax_counts_equal_evaluate_device(trained):
    tr, crops, y = trained["tr"], trained["crops"], trained["y"]
    rows = predict(tr, crops)
    x = torch.from_numpy(crops.astype(F)).cuda()
    t = torch.from_numpy(y.astype(np.int32)).cuda()
    correct = 0
    for k in range(0, 21, MAX_BATCH):
        m = min(MAX_BATCH, 21 - k)
        correct += tr.evaluate_device(x[k:].data_ptr(), t[k:].data_ptr(), m)[1]
    assert int((rows.argmax(axis=1) == y).sum()) == correct


def test_predict_changes_nothing_in_the_trainer(trained):
    tr, ch = trained["tr"], trained["ch"]
    def everything():
        return [tr.read(i, kind, shp).tobytes() for kind in range(4) for i, (_, shp) in enumerate(weights.shapes(P_CLASSES, ch))], tr.steps
    before = everything()
    predict(tr, trained["crops"])
    assert everything() == before


def test_a_following_step_is_the_same_with_and_without_predict(seg, trained):
    ch, precision = trained["ch"], trained["precision"]
    ids = trained["ids"]
    y = ids._labels(MAX_BATCH, 3)
    x = synth(ids, y, 3, ch, False)
    masks = (np.random.default_rng(4).random(MAX_BATCH * 308) >= 0.05).astype(np.uint8)
    losses = []
    for with_predict in (True, False):
        _, tr = make_trainer(seg, ch, precision)
        if with_predict:
            predict(tr, trained["crops"])
        losses.append(tr.step(x, y, masks))
        losses.append(tr.read(22, 0, (P_CLASSES, 100)).tobytes())       # fc2.weight after the step
        tr.close()
    assert losses[0] == losses[2] and losses[1] == losses[3]


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.batches, self.epochs, self.stop_training = [], [], False

    def on_batch_end(self, batch, logs):
        self.batches.append(batch)

    def on_epoch_end(self, epoch, logs):
        self.epochs.append(epoch)


def test_resident_validation_end_to_end(seg):
    ch = 1
    ids, tr = make_trainer(seg, ch, 0)
    val_y = np.repeat(np.arange(P_CLASSES), 4).astype(np.int32)
    val_x = synth(ids, val_y, 11, ch, True)
    uni_y = np.concatenate([np.random.default_rng(k).permutation(P_CLASSES) for k in range(5)]).astype(np.int32)
    uni_x = synth(ids, uni_y, 12, ch, True)
    ranges = np.array([(16 * k, 16 * k + 16) for k in range(5)], np.int32)
    inner = Recorder()
    rv = train_loop.ResidentValidation(tr, seg, val_x, val_y, uni_x, ranges, callback=inner)
    acc = rv.per_class_accuracy()
    rows = seg.copy_to_host(rv.d_probs, (len(val_x), P_CLASSES), F)
    assert rows.tobytes() == predict(tr, val_x).tobytes()
    assert acc.shape == (P_CLASSES,) and np.array_equal(acc, U.per_class_accuracy(rows, val_y, P_CLASSES))
    unique = rv.estimate_uniqueness()
    rows = seg.copy_to_host(rv.d_probs, (len(uni_x), P_CLASSES), F)
    want = U.calculate_uniqueness(rows, [tuple(int(v) for v in r) for r in ranges])
    assert isinstance(unique, float) and unique == rv.last_uniqueness.mean_unique
    held_to_the_bars(rv.last_uniqueness, want, P_CLASSES)
    # ... and as the callback of a resident training run
    train_y = ids._labels(16, 13)
    train = train_loop.ResidentLoader(seg, synth(ids, train_y, 13, ch, True), train_y, batch_size=MAX_BATCH, seed=2)
    val = train_loop.ResidentLoader(seg, val_x[:16], val_y[:16], batch_size=MAX_BATCH, augment=False, shuffle=False)
    hist = train_loop.train_resident(tr, train, val, rv, None, {"epochs": 2})
    assert len(hist) == 2 and inner.epochs == [0, 1] and inner.batches == [0, 1, 0, 1] and not rv.stop_training
    assert len(rv.mean_values) == len(rv.worst_values) == len(rv.uniquenesses) == 2
    assert sorted(rv.per_class_accuracy) == list(range(P_CLASSES)) and all(len(v) == 2 for v in rv.per_class_accuracy.values())
    assert all(0.0 <= v <= 1.0 for v in rv.uniquenesses) and rv.worst_values[-1] <= rv.mean_values[-1]
    inner.stop_training = True
    assert rv.stop_training
    train.close(); val.close(); rv.close(); tr.close()
