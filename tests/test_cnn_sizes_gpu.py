"""The identity network at individual_image_size other than 80x80 on the GPU (the generic chain, cnn_any.hip) against the reference's
own network at those sizes (tests/golden/cnn_v118_3_sizes.npz) and against the CPU oracle.  Bars as in test_cnn_gpu.py: 1e-4 absolute
on softmax, 2e-3 on logits."""
import numpy as np
import pytest
import torch
from oracle import cnn_oracle
from trex_amd import capi, synth, weights
from test_cnn_oracle import load_fixture
from test_cnn_sizes_oracle import CASES, case_id, load_size_case

pytestmark = pytest.mark.gpu

EXACT_MODES = [capi.CNN_FP32, capi.CNN_BF16X6, capi.CNN_FP16X3]


def make_net(st, classes, ch, w, h):
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, classes, ch, w, h))
    assert seg.network_image_size() == (w, h)
    return seg


def run_device(seg, crops, classes):
    n = crops.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(crops)).cuda()
    probs = torch.empty((n, classes), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
    seg.synchronize()
    return probs.cpu().numpy(), logits.cpu().numpy()


@pytest.mark.parametrize("mode", EXACT_MODES + [capi.CNN_BF16X3])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_vectors_at_other_sizes(case, mode):
    w, h, ch, classes, _ = case
    st, want, crops = load_size_case(case)
    seg = make_net(st, classes, ch, w, h)
    seg.set_identity_precision(mode)
    for n, (probs, logits) in want.items():
        p, lg = run_device(seg, crops[n], classes)
        host = seg.probabilities(crops[n])
        assert p.shape == (n, classes) and np.all(np.isfinite(p))
        assert np.abs(host - p).max() <= 1e-6
        assert np.allclose(p.sum(1), 1.0, atol=1e-5)
        if mode == capi.CNN_BF16X3:        # three piece products: reported in test_cnn_gpu.py, not held to the bar
            continue
        assert np.abs(p - probs).max() <= 1e-4, (n, np.abs(p - probs).max())
        assert np.abs(lg - logits).max() <= 2e-3, (n, np.abs(lg - logits).max())
    if mode == capi.CNN_FP16X3:
        assert seg.guard_stats() == (0, False)
    seg.close()


@pytest.fixture(scope="module")
def wide_case():
    """120x16, 1 channel, 8 classes, 33 crops: the only V118_3 case on the 16-wide tile (test_cnn_plan.py::test_any_size) -- conv2 over 4 x 30
    windows, two tiles, ragged in x; conv3 over 2 x 15, one tile, ragged in x and y.  The synthetic ellipse fills 14 % of such a crop, so the
    later half of the crops gets texture on every zero pixel (as cnn_arch_edge_cases.make): a wrong column at the ragged edge must not see
    constant background only.  -> (state, crops, the oracle's probabilities), computed once"""
    w, h, classes, n = 120, 16, 8, 33
    st = weights.synthetic_state(classes, 41, 1, w, h)
    crops = weights.synthetic_crops(n, 1041, 1, w, h)
    late = crops[n // 2:]
    late[late == 0] = np.random.default_rng(2041).integers(1, 256, late.shape, dtype=np.uint8)[late == 0]
    assert (crops[:n // 2] == 0).any() and not (late == 0).any()
    want, _ = cnn_oracle.predict(st, crops, threads=8)
    return st, crops, want


@pytest.mark.parametrize("mode", EXACT_MODES)
def test_the_16_wide_tile_against_the_oracle(wide_case, mode):
    st, crops, want = wide_case
    seg = make_net(st, 8, 1, 120, 16)
    seg.set_identity_precision(mode)
    p, _ = run_device(seg, crops, 8)
    assert p.shape == want.shape and np.all(np.isfinite(p))
    err = np.abs(p - want).max()
    print(f"120x16 mode {mode}: max |dp| = {err:.3g}")
    assert err <= 1e-4, err
    if mode == capi.CNN_FP16X3:
        assert seg.guard_stats() == (0, False)
    seg.close()


@pytest.mark.parametrize("n", [300, 2049])
@pytest.mark.parametrize("size", [(64, 64), (100, 60)])
def test_large_batches_against_the_oracle(size, n):
    w, h = size
    st = weights.synthetic_state(100, 17, 1, w, h)
    crops = weights.synthetic_crops(n, 900 + n, 1, w, h)
    crops[1] = 0
    crops[2] = 255
    seg = make_net(st, 100, 1, w, h)
    p = seg.probabilities(crops)                 # FP16X3, the default
    assert seg.guard_stats() == (0, False)
    rows = np.unique(np.r_[0:40, n - 40:n, 0:n:23])
    want, _ = cnn_oracle.predict(st, crops[rows], threads=16)
    assert np.abs(p[rows] - want).max() <= 1e-4
    seg.set_identity_precision(capi.CNN_FP32)
    assert np.abs(seg.probabilities(crops[rows]) - want).max() <= 1e-4
    seg.close()


def test_replayed_chain_is_bit_identical():
    # the same (buffers, n, precision) key four times and more: captured at the third call, replayed after that
    w = h = 64
    st = weights.synthetic_state(8, 23, 1, w, h)
    seg = make_net(st, 8, 1, w, h)
    n = 100
    crops = torch.from_numpy(weights.synthetic_crops(n, 5, 1, w, h)).cuda()
    probs = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    logits = torch.zeros_like(probs)
    first = None
    for rep in range(6):
        probs.zero_()
        seg.identify_device(crops.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
        seg.synchronize()
        if first is None:
            first = (probs.clone(), logits.clone())
        else:
            assert torch.equal(probs, first[0]) and torch.equal(logits, first[1]), rep
    want, _ = cnn_oracle.predict(st, crops.cpu().numpy()[:16], threads=8)
    assert np.abs(first[0].cpu().numpy()[:16] - want).max() <= 1e-4
    seg.close()


def _conv1_pooled_max(st, crops):
    """largest activation behind conv1 + BN + ReLU + pool per crop (float64): conv2's input, what the fp16 range guard looks at"""
    import torch.nn.functional as F
    t = {k: torch.from_numpy(np.ascontiguousarray(v, np.float64)) for k, v in st.items()}
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(crops)).to(torch.float64).permute(0, 3, 1, 2)
        x = F.conv2d(x, t["conv1.weight"], t["conv1.bias"], padding=2)
        x = F.batch_norm(x, t["bn1.running_mean"], t["bn1.running_var"], t["bn1.weight"], t["bn1.bias"], training=False, eps=1e-5)
        x = F.max_pool2d(F.relu(x), 2)
    return x.reshape(x.shape[0], -1).max(1).values.numpy()


def test_range_guard_reruns_only_the_loud_crop():
    w = h = 96
    st = {k: v.copy() for k, v in weights.synthetic_state(8, 31, 1, w, h).items()}
    n, loud = 300, 117
    rng = np.random.default_rng(5)
    crops = np.zeros((n, h, w, 1), np.uint8)
    crops[:, 24:72, 24:72, 0] = rng.integers(0, 4, (n, 48, 48))           # quiet crops: values 0..3
    quiet_only = crops.copy()
    crops[loud, :, :, 0] = rng.integers(0, 256, (h, w))                    # one loud crop
    base_q, base_l = _conv1_pooled_max(st, quiet_only[:8]).max(), _conv1_pooled_max(st, crops[loud:loud + 1])[0]
    m = 3000.0 / max(base_q, 1e-9)                                         # quiet crops peak at 3000, the loud one beyond fp16
    assert base_l * m > 2 * 65520, (base_q, base_l)
    st["conv1.weight"] *= m; st["conv1.bias"] *= m; st["bn1.running_mean"] *= m
    st["bn2.running_var"] = st["bn2.running_var"] * m * m                 # bring the scale back down behind conv2
    seg = make_net(st, 8, 1, w, h)
    seg.set_identity_precision(capi.CNN_FP16X3)
    a = seg.probabilities(quiet_only)
    assert seg.guard_stats() == (0, False)
    b = seg.probabilities(crops)
    assert seg.guard_stats() == (1, False)
    seg.set_identity_precision(capi.CNN_FP32)
    exact = seg.probabilities(crops[loud:loud + 1])
    assert np.all(np.isfinite(b)) and np.abs(b[loud] - exact[0]).max() <= 1e-4
    others = np.ones(n, bool); others[loud] = False
    assert a[others].tobytes() == b[others].tobytes()                      # untouched by the re-run
    ref, _ = cnn_oracle.predict(st, crops[loud:loud + 1], threads=4)
    assert np.abs(b[loud] - ref[0]).max() <= 1e-4
    seg.close()


def test_reloading_other_sizes_on_one_context():
    z80, st80 = load_fixture(8)
    n80 = 37
    crops80 = weights.synthetic_crops(n80, int(z80["seed"]) + 1000 + n80)
    fresh = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    fresh.load_weights(weights.pack_blob(st80, 8))
    p80_fresh = fresh.probabilities(crops80)
    fresh.close()
    by_size = {(c[0], c[1], c[2]): c for c in CASES}
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    got80 = []
    for size in ((80, 80), (64, 64), (100, 60), (80, 80)):
        if size == (80, 80):
            seg.load_weights(weights.pack_blob(st80, 8))
            assert seg.network_image_size() == (80, 80)
            p = seg.probabilities(crops80)
            assert np.abs(p - z80[f"probs/{n80}"]).max() <= 1e-4
            got80.append(p)
        else:
            case = by_size[size + (1,)]
            st, want, crops = load_size_case(case)
            seg.load_weights(weights.pack_blob(st, case[3], 1, *size))
            assert seg.network_image_size() == size
            for n, (probs, _) in want.items():
                assert np.abs(seg.probabilities(crops[n]) - probs).max() <= 1e-4, (size, n)
    assert got80[0].tobytes() == p80_fresh.tobytes() and got80[1].tobytes() == p80_fresh.tobytes()
    seg.close()


def test_device_chain_at_64x64():
    fr, bg = synth.batch("C2", 2)
    n, H, W = fr.shape
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=n))
    seg.set_background(bg)
    d = torch.from_numpy(fr).to("cuda:0")
    seg.segment_device(d.data_ptr(), n)
    res = seg.fetch()
    classes = 8
    st = weights.synthetic_state(classes, 11, 1, 64, 64)
    seg.load_weights(weights.pack_blob(st, classes, 1, 64, 64))
    nb = sum(len(r.blobs) for r in res)
    assert nb > 0
    crops = torch.zeros((nb, 64, 64), dtype=torch.uint8, device="cuda:0")
    probs = torch.zeros((nb, classes), dtype=torch.float32, device="cuda:0")
    seg.crops_device(crops.data_ptr(), nb, out_w=64, out_h=64)
    seg.identify_device(crops.data_ptr(), nb, probs.data_ptr())
    seg.synchronize()
    c = crops.cpu().numpy()
    assert c.any()
    want, _ = cnn_oracle.predict(st, c[..., None], threads=8)
    assert np.abs(probs.cpu().numpy() - want).max() <= 1e-4
    seg.close()


def test_shapes_and_sizes_are_checked():
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    assert seg.network_image_size() == (0, 0)
    st = weights.synthetic_state(8, 2, 1, 100, 60)
    seg.load_weights(weights.pack_blob(st, 8, 1, 100, 60))
    assert seg.network_image_size() == (100, 60)
    for bad in ((2, 100, 60, 1), (2, 60, 100, 3), (2, 80, 80, 1), (2, 60, 100)):
        with pytest.raises(ValueError):
            seg.probabilities(np.zeros(bad, np.uint8))
    assert seg.probabilities(np.zeros((2, 60, 100, 1), np.uint8)).shape == (2, 8)
    for w, h in ((4, 64), (64, 260)):           # outside 8..256: refused on the header, before the size of the blob is looked at
        blob = bytearray(weights.pack_blob(weights.synthetic_state(8, 2, 1, 64, 64), 8, 1, 64, 64))
        blob[12:20] = np.array([w, h], np.int32).tobytes()
        with pytest.raises(capi.TrexHipError) as e:
            seg.load_weights(bytes(blob))
        assert e.value.code == -4 and "8..256" in str(e.value)
    assert seg.network_image_size() == (100, 60)           # the loaded network stays
    seg.close()
