"""Identity network on the GPU (through the C ABI) vs (a) vectors produced by the reference's own
network module (tests/golden/cnn_v118_3_*.npz) and (b) the CPU oracle.  Tolerance from BASELINE.json:
1e-4 absolute on softmax; logits are also compared (2e-3 abs, |logit| up to ~15)."""
import numpy as np
import pytest
import torch
from oracle import cnn_oracle
from trex_amd import capi, weights
from test_cnn_oracle import load_fixture

pytestmark = pytest.mark.gpu


def make_net(st, classes):
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, classes))
    assert seg.num_classes() == classes
    return seg


@pytest.mark.parametrize("mode", [capi.CNN_FP32, capi.CNN_BF16X6, capi.CNN_FP16X3])
@pytest.mark.parametrize("classes", [8, 100, 256])
def test_reference_vectors(classes, mode):
    z, st = load_fixture(classes)
    seg = make_net(st, classes)
    seg.set_identity_precision(mode)
    sizes = sorted(int(k.split("/")[1]) for k in z.files if k.startswith("probs/"))
    for n in sizes:
        crops = weights.synthetic_crops(n, int(z["seed"]) + 1000 + n)
        probs = seg.probabilities(crops)
        assert probs.shape == (n, classes)
        err = np.abs(probs - z[f"probs/{n}"]).max()
        assert err <= 1e-4, (n, err)
        assert np.allclose(probs.sum(1), 1.0, atol=1e-5)
    seg.close()


@pytest.mark.parametrize("mode", [capi.CNN_FP32, capi.CNN_BF16X6, capi.CNN_FP16X3])
def test_logits_and_device_path_vs_oracle(mode):
    z, st = load_fixture(100)
    seg = make_net(st, 100)
    seg.set_identity_precision(mode)
    rng = np.random.default_rng(5)
    crops = rng.integers(0, 256, (130, 80, 80, 1)).astype(np.uint8)      # dense random crops: worst case for summation order
    crops[7] = 0                                                          # an empty crop
    crops[8] = 255
    d = torch.from_numpy(crops).cuda()
    probs = torch.empty((130, 100), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    seg.identify_device(d.data_ptr(), 130, probs.data_ptr(), logits.data_ptr())
    seg.synchronize()
    op, ol = cnn_oracle.predict(st, crops, threads=8)
    assert np.abs(probs.cpu().numpy() - op).max() <= 1e-4
    assert np.abs(logits.cpu().numpy() - ol).max() <= 2e-3 * max(1.0, np.abs(ol).max() / 10)
    # batch independence: crop 3 alone gives the same row
    one = seg.probabilities(crops[3:4])
    assert np.abs(one[0] - probs[3].cpu().numpy()).max() <= 1e-6
    seg.close()


def test_errors():
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    with pytest.raises(capi.TrexHipError):          # weights not loaded (VisualIdentification.cpp: status().weights.loaded())
        seg.probabilities(np.zeros((1, 80, 80, 1), np.uint8))
    with pytest.raises(capi.TrexHipError):
        seg.load_weights(b"\0" * 64)
    seg.close()


def test_precision_modes_error_ladder():
    """fp32 MFMA and the 6-product bf16 split agree to fp32 rounding; the 3-product split is ~2^-16 per product
    (reported, not asserted against the bar)."""
    z, st = load_fixture(100)
    seg = make_net(st, 100)
    rng = np.random.default_rng(9)
    crops = rng.integers(0, 256, (64, 80, 80, 1)).astype(np.uint8)
    ref, ref_logits = cnn_oracle.predict(st, crops, threads=8)
    errs = {}
    for mode in (capi.CNN_FP32, capi.CNN_BF16X6, capi.CNN_BF16X3, capi.CNN_FP16X3):
        seg.set_identity_precision(mode)
        errs[mode] = float(np.abs(seg.probabilities(crops) - ref).max())
    print("max |dp| vs oracle: fp32 %.3g  bf16x6 %.3g  bf16x3 %.3g  fp16x3 %.3g" % (errs[0], errs[1], errs[2], errs[3]))
    assert errs[capi.CNN_FP32] <= 1e-4 and errs[capi.CNN_BF16X6] <= 1e-4
    assert errs[capi.CNN_BF16X6] <= 20 * max(errs[capi.CNN_FP32], 1e-7)
    assert errs[capi.CNN_FP16X3] <= 20 * max(errs[capi.CNN_FP32], 1e-7)
    seg.close()


def test_fp16_range_overflow_falls_back_on_the_device():
    """Activations beyond the fp16 range (|a| >= 65520) cannot be split into fp16 pieces: the kernel raises a flag and the
    guarded bf16x6 re-run replaces the result -- same answer as the exact path, never a silent inf/NaN."""
    st = weights.synthetic_state(8, 31)
    st = {k: v.copy() for k, v in st.items()}
    st["conv1.weight"] *= 4000.0            # conv1 outputs ~1e5..1e6 => conv2's input leaves the fp16 range
    st["bn1.running_var"] = np.full(16, 1.0, np.float32); st["bn1.running_mean"] = np.zeros(16, np.float32)
    st["bn2.running_var"] = np.full(64, 1e10, np.float32)   # bring the scale back down so later layers stay finite
    crops = weights.synthetic_crops(5, 77)
    ref, _ = cnn_oracle.predict(st, crops, threads=4)
    assert np.all(np.isfinite(ref))
    seg = make_net(st, 8)
    seg.set_identity_precision(capi.CNN_FP16X3)
    got = seg.probabilities(crops)
    assert np.all(np.isfinite(got)) and np.abs(got - ref).max() <= 1e-4
    seg.set_identity_precision(capi.CNN_FP32)
    assert np.abs(seg.probabilities(crops) - ref).max() <= 1e-4
    seg.close()


def _out_of_range_state(channels):
    """the weights of test_fp16_range_overflow_falls_back_on_the_device: every crop's conv1 output leaves the fp16 range, the oracle's rows stay finite"""
    st = {k: v.copy() for k, v in weights.synthetic_state(8, 31, channels=channels).items()}
    st["conv1.weight"] *= 4000.0
    st["bn1.running_var"] = np.full(16, 1.0, np.float32); st["bn1.running_mean"] = np.zeros(16, np.float32)
    st["bn2.running_var"] = np.full(64, 1e10, np.float32)
    return st


def test_three_channel_rerun_starts_at_conv1_on_the_plan():
    """3 channels, FP16X3: the two-kernel chain leaves no fp32 activations, so the guarded re-run starts at the crops (k_conv1_mfma3 on the plan);
    the 3-channel conv1 cannot name the crop that left the range, so the plan orders the whole batch"""
    st = _out_of_range_state(3)
    crops = weights.synthetic_crops(5, 77, channels=3)
    ref, _ = cnn_oracle.predict(st, crops, threads=4)
    assert np.all(np.isfinite(ref))
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, 8, channels=3))
    seg.set_identity_precision(capi.CNN_FP16X3)
    got = seg.probabilities(crops)
    assert np.all(np.isfinite(got)) and np.abs(got - ref).max() <= 1e-4
    assert seg.guard_stats() == (0, True)
    seg.close()


def test_unaligned_rerun_starts_at_conv2():
    """1 channel, FP16X3, crops at an odd device address: the fp32-activation chain, whose guarded re-run keeps conv1's exact act1 and starts at conv2"""
    st = _out_of_range_state(1)
    crops = weights.synthetic_crops(5, 77)
    ref, _ = cnn_oracle.predict(st, crops, threads=4)
    assert np.all(np.isfinite(ref))
    seg = make_net(st, 8)
    raw = torch.zeros(5 * 6400 + 64, dtype=torch.uint8, device="cuda")
    off = (16 - raw.data_ptr() % 16) % 16
    pa = torch.empty((5, 8), dtype=torch.float32, device="cuda"); pb = torch.empty_like(pa)
    raw[off:off + 5 * 6400] = torch.from_numpy(crops.reshape(-1)).cuda()
    seg.set_identity_precision(capi.CNN_FP32)
    seg.identify_device(raw.data_ptr() + off, 5, pa.data_ptr())
    seg.synchronize()
    raw[off + 3:off + 3 + 5 * 6400] = torch.from_numpy(crops.reshape(-1)).cuda()
    seg.set_identity_precision(capi.CNN_FP16X3)
    seg.identify_device(raw.data_ptr() + off + 3, 5, pb.data_ptr())
    seg.synchronize()
    rerun, whole = seg.guard_stats()
    got = pb.cpu().numpy()
    assert np.all(np.isfinite(got)) and np.abs(got - ref).max() <= 1e-4
    assert whole or rerun == 5                  # every crop's conv1 peak is far outside the range
    assert np.abs(got - pa.cpu().numpy()).max() <= 1e-5
    seg.close()


def test_unaligned_crop_buffer_and_both_conv1_kernels_agree():
    # the matrix-core conv1 needs 16-byte aligned crops; an odd device pointer must take the VALU kernel and give the same answer
    z, st = load_fixture(100)
    seg = make_net(st, 100)
    rng = np.random.default_rng(11)
    crops = rng.integers(0, 256, (37, 80, 80, 1)).astype(np.uint8)
    raw = torch.zeros(37 * 6400 + 64, dtype=torch.uint8, device="cuda")
    pa = torch.empty((37, 100), dtype=torch.float32, device="cuda"); pb = torch.empty_like(pa)
    off = (16 - raw.data_ptr() % 16) % 16
    raw[off:off + 37 * 6400] = torch.from_numpy(crops.reshape(-1)).cuda()
    seg.identify_device(raw.data_ptr() + off, 37, pa.data_ptr())
    raw[off + 3:off + 3 + 37 * 6400] = torch.from_numpy(crops.reshape(-1)).cuda()
    seg.identify_device(raw.data_ptr() + off + 3, 37, pb.data_ptr())
    seg.synchronize()
    op, _ = cnn_oracle.predict(st, crops, threads=8)
    assert np.abs(pa.cpu().numpy() - op).max() <= 1e-4 and np.abs(pb.cpu().numpy() - op).max() <= 1e-4
    assert np.abs(pa.cpu().numpy() - pb.cpu().numpy()).max() <= 1e-5
    seg.close()


@pytest.mark.parametrize("n", [1, 2, 127, 129, 255, 257, 300, 515])
def test_batch_sizes_around_the_tile_and_grid_boundaries(n):
    # fc1 works on 128-crop tiles, conv3 on a persistent grid of one workgroup per CU (256), conv2 on 5 workgroups per crop:
    # crop counts around those boundaries must give the same rows as the oracle and as a run of the same crops in another order
    z, st = load_fixture(100)
    seg = make_net(st, 100)
    rng = np.random.default_rng(n)
    crops = weights.synthetic_crops(n, n) if hasattr(weights, "synthetic_crops") else rng.integers(0, 256, (n, 80, 80, 1)).astype(np.uint8)
    p = seg.probabilities(crops)
    op, _ = cnn_oracle.predict(st, crops, threads=8)
    assert p.shape == (n, 100)
    assert np.abs(p - op).max() <= 1e-4
    if n > 2:
        perm = rng.permutation(n)
        p2 = seg.probabilities(crops[perm])
        assert np.abs(p2 - p[perm]).max() <= 1e-6
    seg.close()


@pytest.mark.parametrize("mode", [capi.CNN_FP32, capi.CNN_FP16X3])
def test_three_channel_network(mode):
    # meta_encoding rgb8: V118_3 with 3 input channels (PermuteAxesWrapper: NHWC u8 -> NCHW float, no scaling)
    st = weights.synthetic_state(20, 31, channels=3)
    crops = weights.synthetic_crops(70, 9, channels=3)
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, 20, channels=3))
    seg.set_identity_precision(mode)
    p = seg.probabilities(crops)
    op, _ = cnn_oracle.predict(st, crops, threads=8)
    assert np.abs(p - op).max() <= 1e-4
    seg.close()


def test_replayed_chain_follows_new_inputs_and_precision_changes():
    # small batches replay a captured hipGraph of the identify chain (cnn.hip: net_forward): the replay must see what is in the buffers NOW
    # (crops rewritten in place, the fp16 range flag of THIS batch), and a precision switch must not reuse another mode's chain
    classes, n = 100, 100
    st = weights.synthetic_state(classes, 4242)
    seg = make_net(st, classes)
    crops = torch.zeros((n, 80, 80), dtype=torch.uint8, device="cuda")
    probs = torch.zeros((n, classes), dtype=torch.float32, device="cuda")
    for rep in range(8):                  # (a chain is captured at the third call with the same key: calls 1-2 launch directly, 3 captures, 4+ replay)
        c = weights.synthetic_crops(n, 700 + rep)[..., 0]
        crops.copy_(torch.from_numpy(c).cuda())
        if rep == 6:
            seg.set_identity_precision(capi.CNN_BF16X6)
        seg.identify_device(crops.data_ptr(), n, probs.data_ptr())
        seg.synchronize()
        want, _ = cnn_oracle.predict(st, c[..., None], threads=8)
        assert np.abs(probs.cpu().numpy() - want).max() <= 1e-4, rep
    # a second output buffer and another batch size: their own chains
    probs2 = torch.zeros((37, classes), dtype=torch.float32, device="cuda")
    for rep in range(5):
        seg.identify_device(crops.data_ptr(), 37, probs2.data_ptr())
        seg.synchronize()
        assert np.abs(probs2.cpu().numpy() - want[:37]).max() <= 1e-4
    seg.close()


def test_varying_crop_counts_without_synchronising_between_calls():
    # tracking hands over a different number of crops almost every batch: nothing may be captured for keys seen once or twice, more
    # distinct keys than the cache holds must evict safely although the evicted chains were launched asynchronously, and every call
    # must still give its own crops' rows
    classes = 100
    st = weights.synthetic_state(classes, 99)
    seg = make_net(st, classes)
    allc = weights.synthetic_crops(160, 5)[..., 0]
    want, _ = cnn_oracle.predict(st, allc[..., None], threads=8)
    crops = torch.from_numpy(allc).cuda()
    sizes = [100, 97, 100, 103, 100, 91, 100, 100] + [60 + 3 * k for k in range(12)] * 3 + [100, 100]
    outs = [torch.zeros((160, classes), dtype=torch.float32, device="cuda") for _ in sizes]
    for k, n in enumerate(sizes):          # no synchronisation between the calls
        seg.identify_device(crops.data_ptr(), n, outs[k].data_ptr())
    seg.synchronize()
    for k, n in enumerate(sizes):
        assert np.abs(outs[k][:n].cpu().numpy() - want[:n]).max() <= 1e-4, (k, n)
    # the same key over and over with one output buffer: captured, replayed, still correct
    for _ in range(6):
        seg.identify_device(crops.data_ptr(), 64, outs[0].data_ptr())
    seg.synchronize()
    assert np.abs(outs[0][:64].cpu().numpy() - want[:64]).max() <= 1e-4
    seg.close()


@pytest.mark.parametrize("n", [1, 3, 41, 100, 333, 1000, 2049, 12800])
def test_fused_equals_two_kernel_chain(n, monkeypatch):
    # conv1 inside conv2 (k_conv12_wpre, the default for 1-channel crops) does the arithmetic of k_conv1_wpre + k_conv2_wpre2 in their
    # order: the probabilities are bit-identical to the two-kernel chain (TREXHIP_CONV_GEOM bit 28, read when the context is created).
    # Crop counts around the pass (3 row pairs), ticket (1..16 passes) and chunk boundaries; dense, sparse, empty and saturated crops
    st = weights.synthetic_state(100, 31)
    crops = weights.synthetic_crops(n, 77 + n).copy()
    if n > 2:
        crops[1] = 0; crops[2] = 255
    if n > 40:
        crops[40, 10:30, 5:75] = 0
    out = {}
    # ... and so does the role-split form of the fused kernel (k_conv12_rs: consumer / producer waves in one workgroup, bit 29)
    for name, geom in (("fused", str(1 << 30)), ("two", str(1 << 28)), ("role-split", str(1 << 29))):
        monkeypatch.setenv("TREXHIP_CONV_GEOM", geom)
        seg = make_net(st, 100)
        seg.set_identity_precision(capi.CNN_FP16X3)
        out[name] = seg.probabilities(crops)
        assert seg.guard_stats() == (0, False)
        seg.close()
    assert out["fused"].tobytes() == out["two"].tobytes()
    assert out["role-split"].tobytes() == out["two"].tobytes()
    want, _ = cnn_oracle.predict(st, crops[:64], threads=4)
    assert np.abs(out["fused"][:64] - want).max() <= 1e-4


@pytest.mark.parametrize("geom", [1 << 30, 1 << 29, 0])
def test_large_batch_kernels_repeat_bit_for_bit(geom, monkeypatch):
    """Round 4 found a 1-in-5 schedule hazard (an inline-asm accumulator read that escaped the hazard recognizer) only because one test
    happened to fail; round 5 found the same class again (v_max3 in inline asm on MFMA results: the range guard fired at random).  So the
    large-batch kernels run TEN times here: every repetition of the fused chain (both forms) must reproduce the two-kernel chain's
    probabilities bit for bit, and no repetition may trip the range guard."""
    st = weights.synthetic_state(100, 31)
    n = 12800
    crops = torch.from_numpy(weights.synthetic_crops(n, 77 + n)[..., 0].copy()).cuda()
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(1 << 28))
    seg = make_net(st, 100)
    seg.set_identity_precision(capi.CNN_FP16X3)
    ref = torch.zeros((n, 100), dtype=torch.float32, device="cuda")
    seg.identify_device(crops.data_ptr(), n, ref.data_ptr())
    seg.synchronize()
    seg.close()
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(geom))
    seg = make_net(st, 100)
    seg.set_identity_precision(capi.CNN_FP16X3)
    out = torch.zeros_like(ref)
    for rep in range(10):
        out.zero_()
        seg.identify_device(crops.data_ptr(), n, out.data_ptr())
        assert seg.guard_stats() == (0, False), rep
        assert torch.equal(out, ref), (rep, float((out - ref).abs().max()))
    seg.close()


def _conv1_pooled_max(st, crops):
    """largest activation behind conv1 + BN + ReLU + pool per crop (float64 on the host): what the fp16 range guard of the default chain looks at"""
    w = st["conv1.weight"].astype(np.float64)[:, 0]                      # [16][5][5]
    s = st["bn1.weight"].astype(np.float64) / np.sqrt(st["bn1.running_var"].astype(np.float64) + 1e-5)
    b = (st["conv1.bias"].astype(np.float64) - st["bn1.running_mean"]) * s + st["bn1.bias"]
    out = []
    for c in crops[..., 0].astype(np.float64):
        p = np.pad(c, 2)
        win = np.lib.stride_tricks.sliding_window_view(p, (5, 5))       # [80][80][5][5]
        a = np.einsum("yxij,oij->oyx", win, w) * s[:, None, None] + b[:, None, None]
        out.append(max(a.max(), 0.0))
    return np.array(out)


@pytest.mark.parametrize("geom", [1 << 30, 1 << 29])
def test_range_guard_is_per_crop(geom, monkeypatch):
    """One crop whose conv1 activations leave the fp16-piece range (>= 4368) among quiet ones: only that crop (and at most the neighbours that
    share a pass with it) is re-run by the bf16x6 kernels -- the others keep the bits of a run without it (a whole-batch re-run would move
    them by ~2e-6) -- and the loud crop's answer is the exact path's."""
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(geom))
    st = {k: v.copy() for k, v in weights.synthetic_state(8, 31).items()}
    n, loud = 300, 117
    rng = np.random.default_rng(5)
    crops = np.zeros((n, 80, 80, 1), np.uint8)
    crops[:, 20:60, 20:60, 0] = rng.integers(0, 4, (n, 40, 40))          # quiet crops: values 0..3
    quiet_only = crops.copy()
    crops[loud, :, :, 0] = rng.integers(0, 256, (80, 80))                 # one loud crop
    m = 1.0
    base_q, base_l = _conv1_pooled_max(st, quiet_only[:8]).max(), _conv1_pooled_max(st, crops[loud:loud + 1])[0]
    m = 3000.0 / max(base_q, 1e-9)                                        # quiet crops peak at 3000, the loud one far above 4368
    assert base_l * m > 3 * 4368, (base_q, base_l)
    st["conv1.weight"] *= m; st["conv1.bias"] *= m; st["bn1.running_mean"] *= m
    st["bn2.running_var"] = st["bn2.running_var"] * m * m                 # bring the scale back down behind conv2
    ref, _ = cnn_oracle.predict(st, crops[loud - 2:loud + 3], threads=4)
    seg = make_net(st, 8)
    seg.set_identity_precision(capi.CNN_FP16X3)
    a = seg.probabilities(quiet_only)
    assert seg.guard_stats() == (0, False)
    b = seg.probabilities(crops)
    rerun, whole = seg.guard_stats()
    assert not whole and 1 <= rerun <= 3, (rerun, whole)
    assert np.all(np.isfinite(b)) and np.abs(b[loud - 2:loud + 3] - ref).max() <= 1e-4
    far = np.ones(n, bool); far[loud - 1:loud + 2] = False
    assert a[far].tobytes() == b[far].tobytes()                           # untouched by the re-run
    assert np.abs(a[~far] - b[~far])[[0, 2]].max() <= 1e-5                # the neighbours: re-run or not, the same answer
    seg.close()


def test_unattributed_range_flag_reruns_every_crop(monkeypatch):
    """in the two-kernel chain (TREXHIP_CONV_GEOM bit 28; also the 3-channel network's chain) conv1 / conv2 raise the fp16 range flag
    WITHOUT naming the crop, while fc1 names it.  Crop A leaves the range in conv1, crop B only in front of fc1: a plan that listed just B would
    leave A with its out-of-range fp16 result.  The plan must order every crop, and every row must be the exact path's."""
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(1 << 28))
    st = {k: v.copy() for k, v in weights.synthetic_state(8, 31).items()}
    n, A, B = 40, 11, 29
    rng = np.random.default_rng(9)
    crops = np.zeros((n, 80, 80, 1), np.uint8)
    crops[:, 20:60, 20:60, 0] = rng.integers(0, 4, (n, 40, 40))           # quiet crops
    crops[B, 10:70, 10:70, 0] = rng.integers(0, 12, (60, 60))              # B: brighter, still inside conv1's and conv2's range
    quiet = np.ones(n, bool); quiet[[A, B]] = False
    crops[A, :, :, 0] = rng.integers(0, 256, (80, 80))                     # A: far outside conv1's range
    m1 = cnn_oracle.stage_maxima(st, crops)[0]
    m = 3500.0 / m1[B]                                                      # conv1: B peaks at 3500 (< 4368), A far above
    st["conv1.weight"] *= m; st["conv1.bias"] *= m; st["bn1.running_mean"] *= m
    st["bn2.running_var"] = st["bn2.running_var"] * m * m
    s1, s2, s3 = cnn_oracle.stage_maxima(st, crops)
    assert s1[A] > 3 * 4368 and s1[B] < 4368 and s1[quiet].max() < 4368, (s1[A], s1[B], s1[quiet].max())
    assert s2[B] < 4368 and s2[quiet].max() < 4368, (s2[B], s2[quiet].max())
    # act3 (fc1's input) scaled so that B alone passes what two fp16 pieces hold; fc1 takes the scale back out
    assert s3[B] > 1.25 * s3[quiet].max(), (s3[B], s3[quiet].max())
    M = 80000.0 / s3[B]
    assert s3[quiet].max() * M < 65000
    st["bn3.weight"] *= M; st["bn3.bias"] *= M; st["fc1.weight"] = st["fc1.weight"] / M
    ref, _ = cnn_oracle.predict(st, crops, threads=4)
    seg = make_net(st, 8)
    seg.set_identity_precision(capi.CNN_FP16X3)
    p = seg.probabilities(crops)
    rerun, whole = seg.guard_stats()
    assert whole, (rerun, whole)                                            # not the list {B}
    assert np.all(np.isfinite(p)) and np.abs(p - ref).max() <= 1e-4, np.abs(p - ref).max(1)
    # ... and B alone among quiet crops IS a list (fc1 names its crop)
    only_b = crops.copy(); only_b[A] = only_b[0]
    p2 = seg.probabilities(only_b)
    rerun, whole = seg.guard_stats()
    assert not whole and rerun == 1, (rerun, whole)
    ref2, _ = cnn_oracle.predict(st, only_b, threads=4)
    assert np.abs(p2 - ref2).max() <= 1e-4
    seg.close()


def test_small_batch_kernels_give_the_rows_of_the_large_batch_kernels():
    """up to 1024 crops fc1 takes 32 crops per workgroup and the head one crop per wave (k_fc1_split<1>, k_head_small: TRex's default call is 100
    crops); the same crops inside a larger batch go through k_fc1_split<4> and k_head.  Same sums in the same order: the same bits."""
    z, st = load_fixture(100)
    seg = make_net(st, 100)
    seg.set_identity_precision(capi.CNN_FP16X3)
    crops = weights.synthetic_crops(1100, 77)
    big = seg.probabilities(crops)
    for n in (1, 100, 1000, 1024):
        small = seg.probabilities(crops[:n])
        assert small.tobytes() == big[:n].tobytes(), n
    z256, st256 = load_fixture(256)
    seg2 = make_net(st256, 256)                                            # four 64-class slices
    big = seg2.probabilities(crops)
    assert seg2.probabilities(crops[:100]).tobytes() == big[:100].tobytes()
    seg.close(); seg2.close()
