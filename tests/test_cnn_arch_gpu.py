"""The identity networks v100, v110, v119 and v200 on the GPU (cnn_arch.hip) against the reference's own vectors (tests/golden/cnn_arch.npz)
and the CPU restatement (tests/vi_arch_ref.py).  Bars as in test_cnn_sizes_gpu.py: 1e-4 absolute on softmax, 2e-3 on logits; against float64
the rule of test_cnn_trained_gpu.py: logits within 8 x e32, e32 the float32 restatement's own error on the same crops."""
import numpy as np
import pytest
import torch
from trex_amd import capi, synth, weights
import vi_arch_ref
from vi_arch_ref import ARCHS, CASES, case_id

pytestmark = pytest.mark.gpu

EXACT_MODES = [capi.CNN_FP32, capi.CNN_BF16X6, capi.CNN_FP16X3]
LOGIT_FACTOR = 8.0          # test_cnn_trained_gpu.py
UNDECIDED_CAP = 0.01


def make_net(st, classes, ch, w, h, arch):
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, classes, ch, w, h, arch=arch))
    assert seg.network_image_size() == (w, h) and seg.network_version() == weights.ARCH_IDS[arch] and seg.num_classes() == classes
    return seg


def run_device(seg, crops, classes):
    n = crops.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(crops)).cuda()
    probs = torch.empty((n, classes), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
    seg.synchronize()
    return probs.cpu().numpy(), logits.cpu().numpy()


# ---- 1. the reference's vectors ----
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_reference_vectors(case):
    arch, w, h, ch, classes, _ = case
    st, want, crops = vi_arch_ref.load_case(case)
    seg = make_net(st, classes, ch, w, h, arch)
    assert seg.identify_chunk_crops() >= 1 and seg.skip_stats() == (0, 0, 0) and seg.skip3_stats() == (0, 0, 0, 0)
    for mode in [capi.CNN_BF16X3] + EXACT_MODES:          # (FP16X3 last: its guard statistics are read behind the loop's last call)
        seg.set_identity_precision(mode)
        for n, (probs, logits) in want.items():
            p, lg = run_device(seg, crops[n], classes)
            host = seg.probabilities(crops[n])
            print(case_id(case), "mode", mode, "n", n, "softmax", np.abs(p - probs).max(), "logits", np.abs(lg - logits).max(), "host", np.abs(host - p).max())
            assert p.shape == (n, classes) and np.all(np.isfinite(p)) and np.all(np.isfinite(lg))
            assert np.abs(host - p).max() <= 1e-6
            assert np.allclose(p.sum(1), 1.0, atol=1e-5)
            if mode == capi.CNN_BF16X3:        # three piece products: finite and normalised, not held to the bar
                continue
            assert np.abs(p - probs).max() <= 1e-4, (mode, n, np.abs(p - probs).max())
            assert np.abs(lg - logits).max() <= 2e-3, (mode, n, np.abs(lg - logits).max())
        if mode == capi.CNN_FP16X3:
            assert seg.guard_stats() == (0, False)
    assert seg.skip_stats() == (0, 0, 0) and seg.skip3_stats() == (0, 0, 0, 0)
    seg.close()


# ---- 2. float64 ----
@pytest.mark.parametrize("arch", ARCHS)
def test_logits_against_float64(arch):
    case = [c for c in CASES if c[0] == arch and c[1:4] == (80, 80, 1)][0]
    _, w, h, ch, classes, seed = case
    st, _, _ = vi_arch_ref.load_case(case)
    crops = weights.synthetic_crops(64, seed + 77, ch, w, h)
    _, l64 = vi_arch_ref.forward(st, crops, arch, torch.float64)
    _, l32 = vi_arch_ref.forward(st, crops, arch, torch.float32)
    e32 = float(np.abs(l32 - l64).max())
    top = np.sort(l64, 1)
    decided = (top[:, -1] - top[:, -2]) > 2 * LOGIT_FACTOR * e32
    assert (~decided).mean() <= UNDECIDED_CAP, int((~decided).sum())
    seg = make_net(st, classes, ch, w, h, arch)
    for mode in EXACT_MODES:
        seg.set_identity_precision(mode)
        _, lg = run_device(seg, crops, classes)
        ratio = float(np.abs(lg - l64).max()) / e32
        print(f"{arch} mode {mode}: max |dlogit| = {ratio:.3g} x e32 (e32 = {e32:.3g}), undecided {int((~decided).sum())} of 64")
        assert ratio <= LOGIT_FACTOR, (mode, ratio, e32)
        assert np.array_equal(lg.argmax(1)[decided], l64.argmax(1)[decided])
    seg.close()


# ---- 3. a crop's row does not depend on its chunk ----
@pytest.mark.parametrize("arch", ["v200", "v119"])
def test_rows_do_not_depend_on_the_chunk(arch):
    w = h = 256
    classes = 8
    st = weights.synthetic_state(classes, 61, 1, w, h, arch=arch)
    seg = make_net(st, classes, 1, w, h, arch)
    chunk = seg.identify_chunk_crops()
    assert 1 < chunk < 400, chunk                 # 2 GiB of activations: 26 crops of v200, a few hundred of v119
    n = chunk + 3
    crops = weights.synthetic_crops(n, 62, 1, w, h)
    p, lg = run_device(seg, crops, classes)        # FP16X3, the default
    assert seg.guard_stats() == (0, False)
    rows = [0, chunk - 1, chunk, n - 1]
    for r in rows:
        p1, lg1 = run_device(seg, crops[r:r + 1], classes)
        assert p1.tobytes() == p[r:r + 1].tobytes() and lg1.tobytes() == lg[r:r + 1].tobytes(), r
    want, _ = vi_arch_ref.forward(st, crops[rows], arch, torch.float32, threads=16)
    assert np.abs(p[rows] - want).max() <= 1e-4, np.abs(p[rows] - want).max()
    assert np.all(np.isfinite(p)) and np.allclose(p.sum(1), 1.0, atol=1e-5)
    seg.close()


# ---- 4. the range guard ----
def _first_layer_max(st, crops, arch):
    """largest activation the first matrix-core convolution reads, per crop (float64): what the fp16 range guard looks at"""
    import torch.nn.functional as F
    t = {k: torch.from_numpy(np.ascontiguousarray(v, np.float64)) for k, v in st.items()}
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(crops)).to(torch.float64).permute(0, 3, 1, 2)
        x = F.conv2d(x, t["conv1.weight"], t["conv1.bias"], padding=t["conv1.weight"].shape[-1] // 2)
        bn = lambda y: F.batch_norm(y, t["bn1.running_mean"], t["bn1.running_var"], t["bn1.weight"], t["bn1.bias"], training=False, eps=1e-5)
        x = F.relu(bn(F.max_pool2d(x, 2))) if arch == "v110" else F.relu(bn(x))
    return x.reshape(x.shape[0], -1).max(1).values.numpy()


@pytest.mark.parametrize("arch", ["v110", "v200"])
def test_range_guard_reruns_only_the_loud_crop(arch):
    w = h = 48
    st = {k: v.copy() for k, v in weights.synthetic_state(8, 31, 1, w, h, arch=arch).items()}
    n, loud = 150, 117
    rng = np.random.default_rng(5)
    crops = np.zeros((n, h, w, 1), np.uint8)
    crops[:, 12:36, 12:36, 0] = rng.integers(0, 4, (n, 24, 24))           # quiet crops: values 0..3
    quiet_only = crops.copy()
    crops[loud, :, :, 0] = rng.integers(0, 256, (h, w))                    # one loud crop
    base_q, base_l = _first_layer_max(st, quiet_only[:8], arch).max(), _first_layer_max(st, crops[loud:loud + 1], arch)[0]
    m = 3000.0 / max(base_q, 1e-9)                                         # quiet crops peak at 3000, the loud one beyond fp16
    assert base_l * m > 2 * 65520, (base_q, base_l)
    # scale the first layer's output by m (its BatchNorm's affine), bring the scale back down behind the second convolution
    st["bn1.weight"] *= m; st["bn1.bias"] *= m
    st["bn2.running_var"] = st["bn2.running_var"] * m * m
    st["bn2.running_mean"] = st["bn2.running_mean"] * m
    st["conv2.bias"] *= m
    seg = make_net(st, 8, 1, w, h, arch)
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
    ref, _ = vi_arch_ref.forward(st, crops[loud:loud + 1], arch, torch.float64)
    assert np.abs(b[loud] - ref[0]).max() <= 1e-4
    seg.close()


# ---- 5. reload on one context ----
def test_reloading_versions_on_one_context():
    from test_cnn_oracle import load_fixture
    z80, st80 = load_fixture(8)
    n80 = 37
    crops80 = weights.synthetic_crops(n80, int(z80["seed"]) + 1000 + n80)
    fresh = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    fresh.load_weights(weights.pack_blob(st80, 8))
    assert fresh.network_version() == 0 and fresh.identify_chunk_crops() == 0
    p80_fresh = fresh.probabilities(crops80)
    fresh.close()
    by_arch = {c[0]: c for c in CASES if c[1:4] == (80, 80, 1)}
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    assert seg.network_version() == 0 and seg.identify_chunk_crops() == 0
    got80 = []
    for arch in ("v118_3", "v200", "v110", "v118_3"):
        if arch == "v118_3":
            seg.load_weights(weights.pack_blob(st80, 8))
            assert seg.network_image_size() == (80, 80) and seg.network_version() == 0 and seg.identify_chunk_crops() == 0
            p = seg.probabilities(crops80)
            assert np.abs(p - z80[f"probs/{n80}"]).max() <= 1e-4
            got80.append(p)
        else:
            case = by_arch[arch]
            st, want, crops = vi_arch_ref.load_case(case)
            seg.load_weights(weights.pack_blob(st, case[4], 1, 80, 80, arch=arch))
            assert seg.network_version() == weights.ARCH_IDS[arch] and seg.identify_chunk_crops() > 0
            for n, (probs, _) in want.items():
                assert np.abs(seg.probabilities(crops[n]) - probs).max() <= 1e-4, (arch, n)
    assert got80[0].tobytes() == p80_fresh.tobytes() and got80[1].tobytes() == p80_fresh.tobytes()
    seg.close()


# ---- 6. refusals ----
def test_refusals_leave_the_loaded_network_alone():
    E_INVALID, E_UNSUPPORTED = -1, -4
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    case = [c for c in CASES if c[0] == "v110" and c[1:4] == (8, 8, 1)][0]
    st, want, crops = vi_arch_ref.load_case(case)
    seg.load_weights(weights.pack_blob(st, 8, 1, 8, 8, arch="v110"))

    def header(blob, **kw):
        hdr = np.frombuffer(blob[:32], np.int32).copy()
        for field, v in kw.items():
            hdr[{"width": 3, "height": 4, "arch": 6}[field]] = v
        return hdr.tobytes() + blob[32:]

    v200 = weights.pack_blob(weights.synthetic_state(8, 2, 1, 27, 27, arch="v200"), 8, 1, 27, 27, arch="v200")
    v119 = weights.pack_blob(weights.synthetic_state(8, 2, 1, 16, 16, arch="v119"), 8, 1, 16, 16, arch="v119")
    for blob, code, texts in ((header(v200, width=26), E_UNSUPPORTED, ("v200", "26x27", "minimum 27")),
                              (header(v119, width=15), E_UNSUPPORTED, ("v119", "15x16", "minimum 16")),
                              (header(v200, arch=5), E_INVALID, ("version id 5",))):
        with pytest.raises(capi.TrexHipError) as e:
            seg.load_weights(blob)
        assert e.value.code == code and all(t in str(e.value) for t in texts), str(e.value)
    with pytest.raises(capi.TrexHipError) as e:          # the trainer keeps V118_3
        capi.Trainer(seg, v200, max_batch=8)
    assert e.value.code == E_UNSUPPORTED and "v200" in str(e.value) and "trexhip_trainer_create" in str(e.value), str(e.value)
    assert seg.network_version() == weights.ARCH_IDS["v110"] and seg.network_image_size() == (8, 8)           # the loaded network stays
    assert np.abs(seg.probabilities(crops[37]) - want[37][0]).max() <= 1e-4
    assert capi.lib().trexhip_network_blob_bytes(4, 8, 1, 27, 27) == len(v200) and capi.lib().trexhip_network_blob_bytes(4, 8, 1, 26, 27) == 0
    assert capi.lib().trexhip_network_blob_bytes(0, 8, 1, 80, 80) == len(weights.pack_blob(weights.synthetic_state(8, 2), 8))
    seg.close()


# ---- 7. end to end ----
def test_device_chain_with_a_v110_net():
    fr, bg = synth.batch("C2", 2)
    n, H, W = fr.shape
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=n))
    seg.set_background(bg)
    d = torch.from_numpy(fr).to("cuda:0")
    seg.segment_device(d.data_ptr(), n)
    res = seg.fetch()
    classes = 8
    st = weights.synthetic_state(classes, 11, 1, 64, 64, arch="v110")
    seg.load_weights(weights.pack_blob(st, classes, 1, 64, 64, arch="v110"))
    nb = sum(len(r.blobs) for r in res)
    assert nb > 0
    crops = torch.zeros((nb, 64, 64), dtype=torch.uint8, device="cuda:0")
    probs = torch.zeros((nb, classes), dtype=torch.float32, device="cuda:0")
    seg.crops_device(crops.data_ptr(), nb, out_w=64, out_h=64)
    seg.identify_device(crops.data_ptr(), nb, probs.data_ptr())
    seg.synchronize()
    c = crops.cpu().numpy()
    assert c.any()
    want, _ = vi_arch_ref.forward(st, c[..., None], "v110", torch.float32)
    assert np.abs(probs.cpu().numpy() - want).max() <= 1e-4
    seg.close()
