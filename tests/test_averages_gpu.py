"""Average identity probabilities per individual on the device: trexhip_class_averages_device and train_loop.ResidentAverages against
tests/averages_ref.py (VINetwork::paverages and check_additional_range's arg-max scan, line by line), bit for bit."""
import ctypes as C
import numpy as np
import pytest
import torch

import averages_ref as A
import identity_synth
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


# ---- 1. injected probabilities ------------------------------------------------------------------------------------------------------------
CLASSES = [1, 7, 64, 65, 100, 257]             # one lane, part of a wave, a wave, a wave + 1, two waves in part, five waves
ROWS = [1, 63, 64, 65, 1000, 4099]             # around the 64 rows a wave takes at a time; 4099 > 4096: the rows are cut into two segments
N_IDS = [1, 3, 100]
# every (classes, n) pair with one n_ids each, every n_ids at every classes and every n; then the corners
CASES = [(c, n, N_IDS[(ci + ni) % 3]) for ci, c in enumerate(CLASSES) for ni, n in enumerate(ROWS)] + [(257, 4099, 100), (100, 4099, 3), (1, 4099, 1), (257, 1, 100)]
PATTERNS = ["random", "last_chunk", "one_owner", "alternating"]


def make_probs(n, classes, rng):
    """1.0-scale values mixed with small multiples of 2^-24 (half an ulp of 1.0) and zeros: any re-association of a sum changes bits.
    Normal floats or zero only."""
    big = (rng.random((n, classes)) + 0.5).astype(F)
    small = (rng.integers(1, 8, (n, classes)) * 2.0 ** -24).astype(F)
    kind = rng.random((n, classes))
    out = np.where(kind < 0.35, small, big)
    out = np.where(kind > 0.92, F(0), out).astype(F)
    assert ((out == 0) | (np.abs(out) >= np.finfo(F).tiny)).all()
    return out


def make_keys(pattern, n, n_ids, rng):
    if pattern == "random":                    # key 1 (if there is more than one) gets no rows
        pool = np.array([k for k in range(n_ids) if k != 1 or n_ids == 1])
        return pool[rng.integers(0, len(pool), n)].astype(np.int32)
    if pattern == "last_chunk":                # the last key owns the last rows (at most 5) and nothing else
        last = n_ids - 1
        pool = np.array([k for k in range(n_ids) if k != last] or [last])
        keys = pool[rng.integers(0, len(pool), n)].astype(np.int32)
        keys[-min(n, 5):] = last
        return keys
    if pattern == "one_owner":                 # one key owns every row
        return np.full(n, n_ids // 2, np.int32)
    return (np.arange(n) % min(n_ids, 2)).astype(np.int32)          # strictly alternating


def call(seg, d_probs, n, classes, d_keys, n_ids):
    m = seg.class_averages(d_probs, n, classes, d_keys, n_ids)
    return m.samples.tobytes(), m.values.tobytes(), m.max_index.tobytes(), m.max_p.tobytes()


def want_bytes(probs, keys, n_ids):
    return tuple(np.ascontiguousarray(a).tobytes() for a in A.class_averages(probs, keys, n_ids))


@pytest.mark.parametrize("classes,n,n_ids", CASES)
def test_injected_probabilities_bit_for_bit(seg, classes, n, n_ids):
    rng = np.random.default_rng([classes, n, n_ids])
    probs = make_probs(n, classes, rng)
    d_probs = torch.from_numpy(probs).cuda()
    for pattern in PATTERNS:
        keys = make_keys(pattern, n, n_ids, rng)
        d_keys = torch.from_numpy(keys).cuda()
        got = call(seg, d_probs.data_ptr(), n, classes, d_keys.data_ptr(), n_ids)
        want = want_bytes(probs, keys, n_ids)
        for name, g, w in zip(("samples", "values", "max_index", "max_p"), got, want):
            assert g == w, f"{pattern}: {name} differs"
        assert call(seg, d_probs.data_ptr(), n, classes, d_keys.data_ptr(), n_ids) == got, f"{pattern}: two calls differ"


def test_the_order_of_the_additions_shows(seg):
    """the hand-worked case of tests/test_averages_ref.py on the device: (1 + e) + e = 1, (e + e) + 1 = 1 + 2^-23"""
    e = F(2.0 ** -24)
    probs = np.array([[1, 3], [e, 3], [e, 3], [e, 3], [e, 3], [1, 3]], F)
    keys = np.array([1, 0, 1, 1, 0, 0], np.int32)
    d_probs, d_keys = torch.from_numpy(probs).cuda(), torch.from_numpy(keys).cuda()
    m = seg.class_averages(d_probs.data_ptr(), 6, 2, d_keys.data_ptr(), 2)
    assert m.values[1, 0] == F(1) / F(3) and m.values[0, 0] == (F(1) + F(2.0 ** -23)) / F(3)
    assert m.values[:, 1].tolist() == [3.0, 3.0] and m.samples.tolist() == [3.0, 3.0] and m.max_index.tolist() == [1, 1]


def test_argmax_of_special_rows(seg):
    """a tie (the first index wins), an averaged row of zeros, negative values only, a NaN (never taken), a key without rows"""
    classes = 70
    rows = np.zeros((6, classes), F)
    rows[0, 5] = rows[0, 69] = 0.5; rows[1, 5] = rows[1, 69] = 0.25            # key 0: a tie between class 5 and class 69 (another wave)
    rows[3, :] = -0.5                                                         # key 2: nothing above 0            (key 1: row 2, all zero)
    rows[4, 3] = np.nan; rows[4, 66] = 0.125; rows[4, 67] = 0.125             # key 3: a NaN in front of a tie
    rows[5, :] = np.nan                                                       # key 4: NaN only                   (key 5: no rows)
    keys = np.array([0, 0, 1, 2, 3, 4], np.int32)
    d_rows, d_keys = torch.from_numpy(rows).cuda(), torch.from_numpy(keys).cuda()
    m = seg.class_averages(d_rows.data_ptr(), 6, classes, d_keys.data_ptr(), 6)
    samples, values, max_index, max_p = A.class_averages(rows, keys, 6)
    assert max_index.tolist() == [5, -1, -1, 66, -1, -1] and max_p.tolist() == [0.375, 0, 0, 0.125, 0, 0]
    assert m.max_index.tolist() == max_index.tolist() and m.max_p.tobytes() == max_p.tobytes() and m.samples.tobytes() == samples.tobytes()
    assert np.array_equal(m.values, values, equal_nan=True)                   # the payload of a NaN is not pinned


def test_the_largest_number_of_ids(seg):
    """65536 keys over 20000 rows: the (key, segment) slots are capped (4 segments instead of 5), the scan walks 2^18 entries"""
    n, classes, n_ids = 20000, 2, 65536
    rng = np.random.default_rng(8)
    probs = make_probs(n, classes, rng)
    keys = rng.integers(0, n_ids, n).astype(np.int32)
    keys[:3] = [0, n_ids - 1, 0]
    d_probs, d_keys = torch.from_numpy(probs).cuda(), torch.from_numpy(keys).cuda()
    assert call(seg, d_probs.data_ptr(), n, classes, d_keys.data_ptr(), n_ids) == want_bytes(probs, keys, n_ids)


def test_a_row_base_offset_by_four_bytes(seg):
    classes, n, n_ids = 64, 300, 3
    rng = np.random.default_rng(2)
    probs = make_probs(n, classes, rng)
    keys = make_keys("random", n, n_ids, rng)
    d_keys = torch.from_numpy(keys).cuda()
    buf = torch.zeros(n * classes + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(probs.reshape(-1)).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    aligned = torch.from_numpy(probs).cuda()
    got = call(seg, buf.data_ptr() + 4, n, classes, d_keys.data_ptr(), n_ids)
    assert got == call(seg, aligned.data_ptr(), n, classes, d_keys.data_ptr(), n_ids) == want_bytes(probs, keys, n_ids)


# ---- 2. optional outputs and refusals -------------------------------------------------------------------------------------------------------
def raw_call(seg, d_probs, n, classes, d_keys, n_ids, skip=()):
    """the C call with sentinel-filled outputs -> (return code, {name: array}); the outputs named in `skip` are passed as NULL"""
    k, c = max(n_ids, 1), max(classes, 1)
    out = {"samples": np.full(k, -7, F), "values": np.full((k, c), -7, F), "max_index": np.full(k, -7, np.int32), "max_p": np.full(k, -7, F)}
    ptr = lambda name: None if name in skip else out[name].ctypes.data_as(C.c_void_p)
    rc = capi.lib().trexhip_class_averages_device(seg.handle, C.c_void_p(d_probs), n, classes, C.c_void_p(d_keys), n_ids, ptr("samples"), ptr("values"),
                                                  ptr("max_index"), ptr("max_p"))
    return rc, out


def untouched(out):
    return all((a == -7).all() for a in out.values())


def test_each_output_is_optional(seg):
    classes, n, n_ids = 9, 200, 4
    rng = np.random.default_rng(5)
    probs = make_probs(n, classes, rng)
    keys = make_keys("random", n, n_ids, rng)
    d_probs, d_keys = torch.from_numpy(probs).cuda(), torch.from_numpy(keys).cuda()
    rc, full = raw_call(seg, d_probs.data_ptr(), n, classes, d_keys.data_ptr(), n_ids)
    assert rc == 0 and not any((a == -7).all() for a in full.values())
    names = list(full)
    for skip in [(nm,) for nm in names] + [("samples", "values"), ("values", "max_index", "max_p"), tuple(names)]:
        rc, out = raw_call(seg, d_probs.data_ptr(), n, classes, d_keys.data_ptr(), n_ids, skip=skip)
        assert rc == 0
        for nm in names:
            assert (out[nm] == -7).all() if nm in skip else out[nm].tobytes() == full[nm].tobytes(), (skip, nm)


def test_refusals(seg):
    classes, n, n_ids = 5, 12, 3
    rng = np.random.default_rng(1)
    probs = torch.from_numpy(make_probs(n, classes, rng)).cuda()
    keys = torch.from_numpy(rng.integers(0, n_ids, n).astype(np.int32)).cuda()
    P, K = probs.data_ptr(), keys.data_ptr()
    rc, out = raw_call(seg, P, n, classes, K, n_ids)
    assert rc == 0 and not untouched(out)
    cases = {"n = 0": (P, 0, classes, K, n_ids), "n = -1": (P, -1, classes, K, n_ids), "n = 2^24 + 1": (P, 2 ** 24 + 1, classes, K, n_ids),
             "classes = 0": (P, n, 0, K, n_ids), "classes = 1025": (P, n, 1025, K, n_ids),
             "n_ids = 0": (P, n, classes, K, 0), "n_ids = 65537": (P, n, classes, K, 65537), "no probabilities": (0, n, classes, K, n_ids), "no ids": (P, n, classes, 0, n_ids)}
    for name, args in cases.items():
        rc, out = raw_call(seg, *args)
        assert rc == E_INVALID and untouched(out), name
        assert b"trexhip_class_averages_device" in capi.lib().trexhip_last_error()
    for bad_value in (-1, n_ids):                                              # flagged by the device
        bad = keys.clone()
        bad[7] = bad_value
        rc, out = raw_call(seg, P, n, classes, bad.data_ptr(), n_ids)
        assert rc == E_INVALID and untouched(out), bad_value
        with pytest.raises(capi.TrexHipError):
            seg.class_averages(P, n, classes, bad.data_ptr(), n_ids)
        # and the context goes on
        rc, out = raw_call(seg, P, n, classes, K, n_ids)
        assert rc == 0 and not untouched(out)
        assert out["values"].tobytes() == A.class_averages(probs.cpu().numpy(), keys.cpu().numpy(), n_ids)[1].tobytes()


# ---- 3. end to end on a small trained network ---------------------------------------------------------------------------------------------
P_CLASSES, MAX_BATCH = 16, 8


def synth(ids, labels, seed, ch, u8):
    x = ids.render(labels, seed)
    if ch == 3:
        x = x * np.array([1.0, 0.8, 0.6], F)
    return np.rint(x).astype(np.uint8) if u8 else np.ascontiguousarray(x, F)


def make_trainer(seg, ch, precision):
    """synthetic weights, then two steps on a batch of identity_synth so that the weights are the trainer's own (as tests/test_validation_gpu.py does)"""
    ids = identity_synth.Identities(P_CLASSES, seed=5)
    tr = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(P_CLASSES, 21 + ch, channels=ch), P_CLASSES, ch), max_batch=MAX_BATCH, lr=1e-3, seed=9,
                      precision=precision)
    y = ids._labels(MAX_BATCH, 1)
    x = synth(ids, y, 1, ch, False)
    for _ in range(2):
        tr.step(x, y)
    return ids, tr


@pytest.mark.parametrize("ch,precision", [(1, 0), (1, 1), (3, 0), (3, 1)])
def test_resident_averages_over_the_trainer(seg, ch, precision):
    ids, tr = make_trainer(seg, ch, precision)
    y = ids._labels(21, 2)
    crops = synth(ids, y, 2, ch, True)
    individuals = np.array([40, 7, 7, 12, 40, 40, 3, 7, 12, 40, 3, 3, 7, 40, 12, 7, 7, 40, 3, 12, 90], np.int64)      # any values, not grouped
    before = tr.export()
    ra = train_loop.ResidentAverages(tr.predict_device, seg, crops, individuals)
    assert ra.classes == P_CLASSES
    got = ra.averages()
    rows = seg.copy_to_host(ra.d_probs, (len(crops), P_CLASSES), F)            # the same rows, copied back: the host route
    assert np.abs(rows.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    want = A.paverages(rows, individuals)
    assert list(got) == list(want) == [3, 7, 12, 40, 90]
    for k in want:
        assert got[k][0] == want[k][0] and got[k][1].tobytes() == want[k][1].tobytes(), k
    scan = [A.argmax_scan(want[k][1]) for k in want]
    assert ra.last.max_index.tolist() == [s[0] for s in scan] and ra.last.max_p.tobytes() == np.array([s[1] for s in scan], F).tobytes()
    assert ra.averages()[40][1].tobytes() == got[40][1].tobytes()
    assert tr.export() == before, "the trainer changed"
    ra.close(); tr.close()


def test_resident_averages_over_the_loaded_network_and_device_addresses(seg):
    classes = 8
    seg.load_weights(weights.pack_blob(weights.synthetic_state(classes, 77), classes))
    crops = weights.synthetic_crops(30, 5).reshape(30, 80, 80, 1)
    keys = (np.arange(30) % 5).astype(np.int32)
    keys[keys == 2] = 4                                                        # dense key 2 has no rows
    d_crops, d_keys = torch.from_numpy(crops).cuda(), torch.from_numpy(keys).cuda()
    ra = train_loop.ResidentAverages(seg.identify_device, seg, d_crops.data_ptr(), d_keys.data_ptr(), count=30, id_values=[10, 11, 12, 13, 14])
    assert ra.classes == classes
    got = ra.averages()
    rows = seg.copy_to_host(ra.d_probs, (30, classes), F)
    want = A.paverages(rows, np.array([10, 11, 12, 13, 14])[keys])
    assert list(got) == list(want) == [10, 11, 13, 14]                         # an id without rows is absent
    for k in want:
        assert got[k][0] == want[k][0] and got[k][1].tobytes() == want[k][1].tobytes(), k
    ra.close()
    torch.cuda.synchronize()
