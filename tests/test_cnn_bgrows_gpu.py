"""The windowed instance of the role-split conv1+conv2 kernel makes only the V2 rows (conv1's pooled rows) that have a non-zero crop row under
them and reads the others -- background rows, one constant per channel -- from a row slot it fills from a table made at weight load
(trex_amd/csrc/cnn_skipx.h: skipx_v2_rows, rs_round; cnn_fused12rs.h).  Every result must be, byte for byte, that of a run that makes every
row (TREXHIP_CONV_GEOM bit 22), of a run without windows (bit 23), of a run that computes every pass (bit 27) and of the two-kernel chain
(bit 28).  Bit 29 forces the role-split kernel at small batches."""
import numpy as np
import pytest
import torch
from trex_amd import capi, weights

pytestmark = pytest.mark.gpu

RS = 1 << 29
OTHERS = (("bit 22", RS | 1 << 22), ("bit 23", RS | 1 << 23), ("bit 27", RS | 1 << 27), ("bit 28", 1 << 28))


@pytest.fixture(scope="module")
def state():
    return weights.synthetic_state(100, 31)


def forward(monkeypatch, st, geom, crops, then=None, classes=100):
    """one context under TREXHIP_CONV_GEOM = geom, the crops through identify_device (`then`: other crops written into the same device buffer
    in front of a second call) -> [(probabilities, logits)] per call, guard_stats, [(skipx_stats, bgrow_stats)] per call"""
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(geom))
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, classes))
    seg.set_identity_precision(capi.CNN_FP16X3)
    n = len(crops)
    d = torch.from_numpy(np.ascontiguousarray(crops.reshape(n, -1))).cuda()
    probs = torch.empty((n, classes), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    outs, stats = [], []
    for batch in (crops,) if then is None else (crops, then):
        d.copy_(torch.from_numpy(np.ascontiguousarray(batch.reshape(n, -1))))
        probs.fill_(-1.0); logits.fill_(-1.0)
        seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
        seg.synchronize()
        outs.append((probs.cpu().numpy().copy(), logits.cpu().numpy().copy()))
        stats.append((seg.skipx_stats(), seg.bgrow_stats()))
    guard = seg.guard_stats()
    seg.close()
    return outs, guard, stats


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def blob(crops, i, rows, cols, rng):
    crops[i, rows, cols, 0] = rng.integers(40, 200, crops[i, rows, cols, 0].shape)


def rows_read_and_made(crops):
    """(windowed crops, V2 rows their passes read -- a crop's passes as one run --, those of them with a non-zero crop row under them) from the
    crops' bytes: V3 row r reads the crop rows 4 r - 6 .. 4 r + 9 and the V2 rows 2 r - 2 .. 2 r + 3, V2 row y the crop rows 2 y - 2 .. 2 y + 3,
    conv2 tile t the crop columns 8 t - 6 .. 8 t + 13; a crop whose tiles are at most 8 has a window"""
    windowed = read = made = 0
    for c in crops:
        c = c.reshape(80, 80)
        ys, xs = np.flatnonzero(c.any(1)), np.flatnonzero(c.any(0))
        if not len(ys):
            continue
        tiles = [t for t in range(10) if 8 * t + 13 >= xs[0] and 8 * t - 6 <= xs[-1]]
        if len(tiles) > 8:
            continue
        windowed += 1
        v3 = [r for r in range(20) if 4 * r + 9 >= ys[0] and 4 * r - 6 <= ys[-1]]
        v2 = [y for y in range(2 * v3[0] - 2, 2 * v3[-1] + 4) if 0 <= y < 40]
        read += len(v2)
        made += sum(1 for y in v2 if 2 * y + 3 >= ys[0] and 2 * y - 2 <= ys[-1])
    return windowed, read, made


def check(monkeypatch, st, crops, then=None):
    """-> [(skipx_stats, bgrow_stats)] per call of the default run, held byte for byte to the four others"""
    on, g_on, s_on = forward(monkeypatch, st, RS, crops, then)
    assert g_on == (0, False)
    for out in on:
        assert np.all(np.isfinite(out[0])) and np.allclose(out[0].sum(1), 1.0, atol=1e-5)
    for name, geom in OTHERS:
        other, g_other, s_other = forward(monkeypatch, st, geom, crops, then)
        assert g_other == (0, False), name
        for call, (a, b) in enumerate(zip(on, other)):
            assert same(a, b), (name, call, float(np.abs(a[1] - b[1]).max()), np.flatnonzero(np.any(a[1] != b[1], axis=1))[:10])
        if name == "bit 22":
            assert [s[0] for s in s_other] == [s[0] for s in s_on]          # the same windows and passes
            assert all(s[1] == (0, 0) for s in s_other)
        if name == "bit 23":
            assert all(s == ((0, 0, 0), (0, 0)) for s in s_other)
    return s_on


def test_one_pixel_in_each_row(monkeypatch, state):
    """80 crops, one pixel in row r: a range that is off by one at either end makes a background row of a row with the pixel under it.  The
    columns spread the crops over all three t0"""
    crops = np.zeros((80, 80, 80, 1), np.uint8)
    for r in range(80):
        crops[r, r, (37 * r + 11) % 80, 0] = 255
    t0 = {min(max(0, -(-(((37 * r + 11) % 80) - 13) // 8)), 2) for r in range(80)}
    assert t0 == {0, 1, 2}
    (skipx, bg), = check(monkeypatch, state, crops)
    want = rows_read_and_made(crops)
    assert skipx == (80, 80, 0) and want[0] == 80
    assert bg == want[1:] and 0 < bg[1] < bg[0]
    # a pixel in row r has 3 V2 rows over it (2 y - 2 <= r <= 2 y + 3), 2 at the crop's first and last two rows
    assert bg[1] == 3 * 76 + 2 * 4


def test_chunk_boundaries(monkeypatch, state):
    rng = np.random.default_rng(8)
    crops = np.zeros((6, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(30, 42), slice(20, 40), rng)         # V2 rows 14 .. 21 made: pass 0 (V3 6 .. 9) makes exactly 8, pass 1 (10, 11) none: halo only
    blob(crops, 1, slice(0, 21), slice(30, 50), rng)          # from row 0: pass 0 reads V2 rows 0 .. 9 and makes all 10: two chunks
    blob(crops, 2, slice(0, 19), slice(30, 50), rng)          # V2 rows 0 .. 10 made; V3 rows 0 .. 6
    blob(crops, 3, slice(0, 80), slice(40, 60), rng)          # every row
    blob(crops, 4, slice(10, 11), slice(5, 9), rng)           # first needed V3 row 1: pass 0 reads V2 rows 0 .. 11, makes 4 .. 6
    blob(crops, 5, slice(14, 40), slice(60, 80), rng)         # first needed V3 row 2: reads 2 .. 13, makes 6 .. 13: exactly 8
    (skipx, bg), = check(monkeypatch, state, crops)
    assert skipx[0] == 6 and skipx[2] == 0
    assert bg == rows_read_and_made(crops)[1:]


def test_blobs_at_row_0_and_row_79(monkeypatch, state):
    rng = np.random.default_rng(9)
    crops = np.zeros((6, 80, 80, 1), np.uint8)
    blob(crops, 0, slice(0, 1), slice(0, 58, 11), rng)        # row 0 alone, tiles 0 .. 7
    blob(crops, 1, slice(79, 80), slice(14, 60, 7), rng)      # row 79 alone, tiles 1 .. 7
    blob(crops, 2, slice(0, 12), slice(0, 9), rng)
    blob(crops, 3, slice(68, 80), slice(71, 80), rng)
    crops[4, 0, 40, 0] = 1; crops[4, 79, 41, 0] = 1          # rows 0 and 79 and nothing between: every row is made
    blob(crops, 5, slice(1, 79), slice(38, 44), rng)          # every row but the first and the last
    (skipx, bg), = check(monkeypatch, state, crops)
    assert skipx[0] == 6 and skipx[2] == 0
    assert bg == rows_read_and_made(crops)[1:]


def test_t0_variants_between_an_empty_and_a_noise_crop(monkeypatch, state):
    """consecutive crops with t0 = 0, 1, 2, 0, ...: blobs at column 0 (tile 0's zero padding) and at column 79 (tile 9's), short in y so that
    every pass reads background rows above and below"""
    rng = np.random.default_rng(10)
    crops = np.zeros((11, 80, 80, 1), np.uint8)
    cols = (slice(0, 10), slice(14, 66), slice(70, 80))        # t0 = 0; tiles 1 .. 8: t0 = 1; t0 = 2
    at = [0, 1, 2, 4, 5, 6, 8, 9, 10]                           # crop 3 stays empty, crop 7 is noise: no window
    for k, i in enumerate(at):
        y = (38, 3, 70, 20, 55, 0, 76, 47, 12)[k]
        blob(crops, i, slice(y, y + 4), cols[k % 3], rng)
    crops[7, :, :, 0] = rng.integers(1, 256, (80, 80))
    (skipx, bg), = check(monkeypatch, state, crops)
    assert skipx[0] == 9 and skipx[2] >= 7
    assert bg == rows_read_and_made(crops)[1:] and bg[1] < bg[0]


def test_t0_changes_inside_a_ticket(monkeypatch, state):
    """three crops per CU, one pass each, t0 = 0, 1, 2, 0, ...: a ticket is several list slots (cnn_plan.h), so a workgroup goes from one
    first tile to another between two passes and its background slot has to follow"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * cus
    assert (20 * n + 2) // 3 // (4 * cus) >= 2, (cus, n)
    rng = np.random.default_rng(11)
    crops = np.zeros((n, 80, 80, 1), np.uint8)
    cols = (slice(0, 10), slice(14, 66), slice(70, 80))
    for i in range(n):
        y = 12 + (7 * i) % 56                                   # rows y .. y + 3: V3 rows within one pass of 4, background rows either side
        blob(crops, i, slice(y, y + 4), cols[i % 3], rng)
    (skipx, bg), = check(monkeypatch, state, crops)
    want = rows_read_and_made(crops)
    assert skipx[0] == n and skipx[2] == 0 and skipx[1] <= 2 * n
    assert bg == want[1:] and bg[1] < bg[0]


def test_tickets_of_two_slots(monkeypatch, state):
    """ellipses at every angle, as many that a ticket is two list slots (cnn_plan.h): a pass that does not follow its predecessor -- a ticket's
    first -- makes its rows again and must not take the previous crop's from the ring"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (8 * cus * 3 + 19) // 20 + 12
    assert min(32, (20 * n + 2) // 3 // (4 * cus)) == 2, (cus, n)
    crops = weights.synthetic_crops(n, 4321).copy()
    crops[17] = 0
    crops[200, :, :, 0] = np.random.default_rng(1).integers(1, 256, (80, 80))
    (skipx, bg), = check(monkeypatch, state, crops)
    want = rows_read_and_made(crops)
    print("%d crops, %d windowed: %d V2 rows read, %d made (%.3f)" % (n, skipx[0], bg[0], bg[1], bg[1] / max(bg[0], 1)))
    assert skipx[0] == want[0] and bg == want[1:] and 0 < bg[1] < bg[0]


def test_two_calls_on_one_context(monkeypatch, state):
    """other crops in the same buffer: ranges, lists and counters follow the bytes that are there now"""
    n = 24
    crops = weights.synthetic_crops(n, 555).copy()
    other = np.zeros_like(crops)
    other[:, 50:70] = weights.synthetic_crops(n, 556)[:, 30:50]
    other[3] = 0
    first, second = check(monkeypatch, state, crops, then=other)
    assert first[1] == rows_read_and_made(crops)[1:] and second[1] == rows_read_and_made(other)[1:]
    assert first[1] != second[1]


def test_background_out_of_range(monkeypatch, state):
    """conv1's bias so large that the background row itself leaves what two fp16 pieces hold: no crop has a window, nobody reads a
    background slot, the counters stay 0"""
    st = {k: v.copy() for k, v in state.items()}
    st["bn1.bias"] = np.full(16, 6000.0, np.float32)
    st["bn2.running_var"] = np.full(64, 1e8, np.float32)
    crops = weights.synthetic_crops(9, 99).copy()
    crops[4] = 0
    on, g_on, s_on = forward(monkeypatch, st, RS, crops)
    assert np.all(np.isfinite(on[0][0]))
    assert s_on[0] == ((0, 0, 60), (0, 0))
    for name, geom in OTHERS:
        other, g_other, s_other = forward(monkeypatch, st, geom, crops)
        assert (g_on[1] or g_on[0] > 0) and (g_other[1] or g_other[0] > 0), (name, g_on, g_other)
        assert same(on[0], other[0]), (name, float(np.abs(on[0][1] - other[0][1]).max()))
        assert s_other[0][1] == (0, 0), name
