"""fc1 (k_fc1_split<4>) computes only the (crop, split-K plane) rows whose row pair conv3's rule lists, the head takes every other plane from the
fc1 planes of an all-zero crop, and k_act3_fill no longer copies the unlisted pairs (trex_amd/csrc/cnn_skip3.h: skip3_fc1_listed): every result
must be, bit for bit, that of the same call with the dense fc1 (TREXHIP_CONV_GEOM bit 24) and that of the two-kernel chain (bit 28), the range
guard must re-run the same crops, and fc1_stats() must say what the crops in the test say.  Bit 29 forces the role-split chain; 1025 crops is
the smallest batch that takes k_fc1_split<4> and k_head: eight full tiles of 128 crops and one crop in a ninth."""
import os
import numpy as np
import pytest
import torch
from trex_amd import capi, weights

pytestmark = pytest.mark.gpu

N = 1025
ON, OFF, TWO = 1 << 29, 1 << 29 | 1 << 24, 1 << 28


@pytest.fixture(scope="module")
def state():
    return weights.synthetic_state(100, 31)


@pytest.fixture(scope="module")
def blobs():
    """N + 64 blob crops, made once; the tests copy what they take"""
    return weights.synthetic_crops(N + 64, 2025)


def forward(monkeypatch, st, geom, batches, classes=100):
    """one context, the same device buffers in every call: -> per call ((probabilities, logits), guard_stats, fc1_stats)"""
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(geom))
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, classes))
    seg.set_identity_precision(capi.CNN_FP16X3)
    n = len(batches[0])
    d = torch.empty((n, 80 * 80), dtype=torch.uint8, device="cuda")
    probs = torch.empty((n, classes), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    out = []
    for crops in batches:
        assert len(crops) == n
        d.copy_(torch.from_numpy(np.ascontiguousarray(crops.reshape(n, -1))))
        probs.fill_(-1.0); logits.fill_(-1.0)
        seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
        seg.synchronize()
        out.append(((probs.cpu().numpy().copy(), logits.cpu().numpy().copy()), seg.guard_stats(), seg.fc1_stats()))
    seg.close()
    return out


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def pairs_of(crop):
    """the row pairs (= fc1 planes) of a crop that read one of its non-zero rows: pair q reads the crop rows 8 q - 14 .. 8 q + 21"""
    rows = np.flatnonzero(crop.reshape(80, -1).any(1))
    return [q for q in range(10) if len(rows) and rows[0] <= 8 * q + 21 and rows[-1] >= 8 * q - 14]


def plane_lengths(crops):
    return [sum(q in pairs_of(c) for c in crops) for q in range(10)]


def check(monkeypatch, st, batches, every_pair=False, guard=(0, False), two_kernel=True):
    """the listed fc1 against the dense one and the two-kernel chain, call by call -> the listed run"""
    on = forward(monkeypatch, st, ON, batches)
    off = forward(monkeypatch, st, OFF, batches)
    two = forward(monkeypatch, st, TWO, batches) if two_kernel else off
    for k, crops in enumerate(batches):
        (r_on, g_on, f_on), (r_off, g_off, f_off), (r_two, g_two, f_two) = on[k], off[k], two[k]
        want = (10 * len(crops), 10 * len(crops) if every_pair else sum(len(pairs_of(c)) for c in crops))
        print("call %d: fc1_stats %s (want %s), guard %s / %s / %s, max |dlogit| vs dense fc1 %.3g, vs two-kernel %.3g"
              % (k, f_on, want, g_on, g_off, g_two, float(np.abs(r_on[1] - r_off[1]).max()), float(np.abs(r_on[1] - r_two[1]).max())))
        assert np.all(np.isfinite(r_on[0])) and np.allclose(r_on[0].sum(1), 1.0, atol=1e-5)
        assert same(r_on, r_off), k
        assert same(r_on, r_two), k
        assert g_on == g_off == g_two, k
        if guard is not None:
            assert g_on == guard, k
        assert f_on == want, k
        assert f_off == (0, 0) and f_two == (0, 0), k
    return on


def one_pixel(row, col=None):
    c = np.zeros((80, 80, 1), np.uint8)
    c[row, (37 * row + 11) % 80 if col is None else col, 0] = 255
    return c


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 80, 80, 1)).astype(np.uint8)


def mixed(blobs, seed):
    rng = np.random.default_rng(seed)
    crops = blobs[:N].copy()
    crops[3] = 0
    crops[4] = noise(1, seed)[0]
    for r in range(80):                                   # a pixel in row r: a plane off by one in either direction at any row shows
        crops[200 + 7 * r] = one_pixel(r)
    crops[9] = 0; crops[9, 0:9, 20:60, 0] = rng.integers(40, 200, (9, 40))          # touches row 0
    crops[1024] = 0; crops[1024, 70:80, 5:75, 0] = rng.integers(40, 200, (10, 70))   # touches row 79, alone in the ninth tile
    return crops


def test_mixed_batch(monkeypatch, state, blobs):
    crops = mixed(blobs, 1)
    assert pairs_of(crops[3]) == [] and pairs_of(crops[4]) == list(range(10)) and pairs_of(crops[9]) == [0, 1, 2] and pairs_of(crops[1024]) == [7, 8, 9]
    assert {len(pairs_of(crops[200 + 7 * r])) for r in range(80)} == {2, 3, 4, 5}
    on = check(monkeypatch, state, [crops])
    rows, listed = on[0][2]
    assert rows // 4 < listed < rows


def test_plane_lengths_at_the_edges(monkeypatch, state):
    """one-pixel crops among empty ones: row 0 lists planes 0, 1; row 2 planes 0, 1, 2; row 77 planes 7, 8, 9; row 79 planes 8, 9 -- so that
    planes 3 .. 6 are listed by no crop, plane 2 by exactly one, plane 7 by 127, planes 0 and 1 by 128 and planes 8 and 9 by 129"""
    kinds = [0] * 127 + [2] + [77] * 127 + [79] * 2
    rng = np.random.default_rng(3)
    where = np.sort(rng.choice(N, len(kinds), replace=False))
    rows = rng.permutation(kinds)
    crops = np.zeros((N, 80, 80, 1), np.uint8)
    for i, r in zip(where, rows):
        crops[i] = one_pixel(int(r), int(rng.integers(0, 80)))
    assert plane_lengths(crops) == [128, 128, 1, 0, 0, 0, 0, 127, 129, 129]
    check(monkeypatch, state, [crops])


def test_stale_buffers(monkeypatch, state, blobs):
    """a noise call writes every pair of act3 and every plane of fc1; the sparse call behind it in the same buffers must read none of what it
    left where its own pairs are not listed -- and the reverse: behind a sparse call the noise call finds stale rows everywhere"""
    sparse = mixed(blobs, 2)
    full = noise(N, 5)
    check(monkeypatch, state, [full, sparse])
    check(monkeypatch, state, [sparse, full, sparse[::-1]])


def test_through_the_captured_graph(monkeypatch, state, blobs):
    """five calls with the same key -- the chain is captured at the third and replayed from the fourth on -- with other crops in the buffer
    every time: the lists are made inside the chain and follow the bytes"""
    assert os.environ.get("TREXHIP_GRAPHS", "1") != "0"
    base = mixed(blobs, 4)
    cut = np.zeros_like(base)
    cut[:, 30:50] = blobs[64:N + 64][:, 30:50]            # every blob cut down to rows 30 .. 49: fewer planes
    batches = [base, np.roll(base, 17, axis=0), cut, np.roll(base, 11, axis=1), np.roll(cut, 25, axis=1)]
    on = check(monkeypatch, state, batches)
    listed = [f[1] for _, _, f in on]
    assert len(set(listed)) > 2 and listed[0] == listed[1] and listed[2] < listed[0]


def test_background_out_of_range_for_fc1_only(monkeypatch, state, blobs):
    """conv3's bias of one channel so large that the empty crop's act3 leaves what two fp16 pieces hold (65520) while V3 stays in range: the
    empty crop's fc1 planes are not used, every pair is listed, and the range guard does what it does with the dense fc1"""
    st = {k: v.copy() for k, v in state.items()}
    ch = int(np.argmax(st["bn3.weight"]))
    assert st["bn3.weight"][ch] >= 1.0
    st["conv3.bias"][ch] = 1e5
    on = check(monkeypatch, st, [mixed(blobs, 6)], every_pair=True, guard=None)
    g = on[0][1]
    assert g[1] or g[0] > 0, g                            # every crop carries the value: the guard re-runs


def test_per_crop_rerun(monkeypatch, state, blobs):
    """a handful of bright crops among dim ones, conv1 scaled (with what follows it: the BN statistics) until the bright ones leave the fp16
    range and the guard re-runs them, crop by crop, in bf16x6: their rows, and everyone else's, are those of the run with the dense fc1"""
    crops = (mixed(blobs, 7) >> 4).astype(np.uint8)       # dim: at most 15
    # (the fused conv1 + conv2 kernel attributes a value to the crops that share its pass of three V3 rows, 20 rows to a crop: blocks that
    # begin and end at a multiple of three crops share no pass with a dim neighbour, so every chain names the same crops)
    bright = [0, 1, 2, 129, 130, 131, 1023, 1024]
    for i, c in zip(bright, noise(len(bright), 9)):
        crops[i] = c | 0xf0                               # at least 240

    def scaled(m):
        st = {k: v.copy() for k, v in state.items()}
        st["conv1.weight"] *= m; st["conv1.bias"] *= m; st["bn1.running_mean"] *= m
        st["bn2.running_var"] = st["bn2.running_var"] * m * m
        return st

    m, g = 4.0, (0, False)
    for _ in range(12):                                   # the bright crops are 16 times the dim ones: one of these steps of 2 trips only them
        g = forward(monkeypatch, scaled(m), ON, [crops])[0][1]
        if g != (0, False):
            break
        m *= 2.0
    print("conv1 scaled by %g: guard %s" % (m, g))
    assert not g[1] and 0 < g[0] <= len(bright), (m, g)
    # (not against the two-kernel chain here: its conv1 is a kernel of its own that raises the flag without naming a crop, so that chain re-runs
    # the whole batch in bf16x6 -- guard (0, True) -- and every row differs from the fp16x3 one by about 1e-5 on the logits, with or without this list)
    check(monkeypatch, scaled(m), [crops], guard=g, two_kernel=False)
