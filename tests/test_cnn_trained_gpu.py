"""The identity network on TRAINED weights, through the C ABI, against the float64 oracle (oracle/cnn_oracle.py, dtype=torch.float64).

Every other CNN test builds its network from weights.synthetic_state: random-init weights, BatchNorm statistics from one calibration pass,
a softmax made peaky by hand.  A trained network is sure of itself (large logits, saturated softmax), its BatchNorm statistics and
LayerNorm gains are far from their initial values, and its activations are what the fp16 range guards of the default chain really see.
tests/trained_net.py trains one with the project's own trainer on the synthetic identities of tests/identity_synth.py (once per process);
the weights are only inputs -- every expectation below is computed from the same weights by the float64 oracle, and every bound from the
error an honest fp32 evaluation (the fp32 oracle) makes against it, never from the device.

Measured figures (MI355X) are recorded in DESIGN.md section 4; the tests print them (run with -s).
"""
import functools
import os
import numpy as np
import pytest
import torch

from trex_amd import capi, weights
import identity_synth
import trained_net

pytestmark = pytest.mark.gpu

MODES = [(capi.CNN_FP32, "fp32"), (capi.CNN_BF16X6, "bf16x6"), (capi.CNN_BF16X3, "bf16x3"), (capi.CNN_FP16X3, "fp16x3")]
LOGIT_FACTOR = 8.0          # device logits within 8 x e32 of the float64 ones: another summation order over 1600 .. 12800 terms
UNDECIDED_CAP = 0.01        # at most 1 % of the crops may be left out of an arg-max / guard statement
LIMITS = (4368.0, 4368.0, 65520.0)   # fp16x3 range: behind conv1, in front of conv3, in front of fc1
BAND = 0.005                # +-0.5 % around each limit: the device compares ITS activation, the host the oracle's
FB_MAX = 1024               # cnn.hip: more flagged crops than this and every crop is re-run
STATS = os.path.join(os.path.dirname(__file__), "golden", "cnn_trained_stats.npz")


def make_net(blob):
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(blob)
    return seg


def device_forward(seg, crops):
    """identify_device on device buffers -> (softmax, logits) as float32 ndarrays"""
    n = len(crops)
    d = torch.from_numpy(np.ascontiguousarray(crops[..., 0])).cuda()
    probs = torch.empty((n, seg.num_classes()), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
    seg.synchronize()
    return probs.cpu().numpy(), logits.cpu().numpy()


def top_two_gap(logits):
    s = np.sort(logits, 1)
    return s[:, -1] - s[:, -2]


def check_rows(tag, probs, logits, p64, l64, e32, hold_logits=True, cap=True):
    """the bars of part (a) on a set of rows; -> the logit error as a multiple of e32.  cap: at most 1 % of the rows may be left out of the
    arg-max statement (the parity set of a trained net; not a handful of rows picked because their activations are extreme)"""
    assert np.all(np.isfinite(probs)) and np.all(np.isfinite(logits)), tag
    dp = float(np.abs(probs - p64).max())
    ds = float(np.abs(probs.astype(np.float64).sum(1) - 1.0).max())
    ratio = float(np.abs(logits - l64).max()) / e32
    gap = top_two_gap(l64)
    decided = gap > 2 * LOGIT_FACTOR * e32
    wrong = int((logits.argmax(1) != l64.argmax(1))[decided].sum())
    print(f"{tag}: max |dp| {dp:.3g}, max |row sum - 1| {ds:.3g}, max |dlogit| = {ratio:.3g} x e32 (e32 = {e32:.3g}, max |logit| {np.abs(l64).max():.4g}), "
          f"arg-max undecided {int((~decided).sum())} of {len(gap)}, wrong {wrong}")
    assert dp <= 1e-4, (tag, dp)
    assert ds <= 1e-5, (tag, ds)
    if hold_logits:
        assert ratio <= LOGIT_FACTOR, (tag, ratio)
        assert not cap or (~decided).mean() <= UNDECIDED_CAP, (tag, float((~decided).mean()))
        assert wrong == 0, (tag, wrong)
    return ratio


@functools.lru_cache(maxsize=None)
def parity_set():
    """2048 test-set crops + the edge crops, their float64 softmax / logits, and e32 = max |fp32-torch logits - float64 logits| on them"""
    acc, top = trained_net.assert_trained()
    st, _ = trained_net.trained_state()
    x, y, p64, l64 = trained_net.held_out_reference()
    edge = identity_synth.edge_crops(trained_net.identities())
    pe, le = trained_net.oracle_f64(st, edge)
    crops, p64, l64 = np.concatenate([x, edge]), np.concatenate([p64, pe]), np.concatenate([l64, le])
    l32 = trained_net.oracle_f32_logits(st, crops)
    e32 = float(np.abs(l32 - l64).max())
    print(f"trained net: test accuracy {acc:.4f}, mean top softmax {top:.4f}, e32 = {e32:.3g}")
    return crops, p64, l64, l32, e32


# ---- the training run itself ---------------------------------------------------------------------------------------------------------

def test_training_run_lies_within_the_reference_modules_seed_spread():
    """Several hundred steps of the device trainer learn what the reference's own module + torch.optim.Adam learn on the same stream: final
    validation loss and test accuracy within the range of the three reference runs (three dropout seeds, tests/golden/cnn_trained_stats.npz),
    widened by that range's own width on each side (and by at least 0.02 in accuracy) -- the spread between dropout seeds is the only
    honest yardstick for two runs that draw different masks.  The training loss falls from epoch to epoch over the first epochs, as the
    generator asserted of all three reference runs."""
    acc, top = trained_net.assert_trained()
    _, hist = trained_net.trained_state()
    z = np.load(STATS)
    assert [int(v) for v in z["meta"]] == [trained_net.CLASSES, trained_net.IDENTITY_SEED, trained_net.WEIGHT_SEED, trained_net.EPOCHS,
                                           identity_synth.BATCHES_PER_EPOCH, identity_synth.BATCH, trained_net.MONO_EPOCHS], "fixture made by another recipe"
    assert len(hist) == trained_net.EPOCHS
    ref_loss, ref_acc = z["history"][:, -1, 1], z["test_accuracy"]
    wl, wa = float(np.ptp(ref_loss)), max(float(np.ptp(ref_acc)), 0.02)
    val_loss = hist[-1]["val_loss"]
    print(f"device run: final val loss {val_loss:.4f} (reference seeds {np.round(ref_loss, 4)}), test accuracy {acc:.4f} (reference {np.round(ref_acc, 4)}), "
          f"val accuracy {hist[-1]['val_acc']:.4f}, training loss per epoch {[round(h['loss'], 4) for h in hist]}")
    assert ref_loss.min() - wl <= val_loss <= ref_loss.max() + wl, (val_loss, ref_loss)
    assert ref_acc.min() - wa <= acc <= ref_acc.max() + wa, (acc, ref_acc)
    loss = np.array([h["loss"] for h in hist])
    assert np.all(np.diff(loss[:trained_net.MONO_EPOCHS]) < 0), loss


def test_training_twice_gives_the_same_bits_and_the_blob_round_trips():
    """every reduction of the trainer has a fixed order and the library-drawn masks a fixed seed: a second full run exports the same blob;
    and that blob survives unpack_blob / pack_blob and tools/convert_weights.py (the way a real checkpoint comes in) bit for bit"""
    blob, hist = trained_net.trained_blob()
    blob2, hist2 = trained_net.trained_blob.__wrapped__()
    assert blob2 == blob
    assert [(h["loss"], h["val_loss"]) for h in hist2] == [(h["loss"], h["val_loss"]) for h in hist]
    st, c, ch = weights.unpack_blob(blob)
    assert weights.pack_blob(st, c, ch) == blob
    import importlib.util
    spec = importlib.util.spec_from_file_location("convert_weights", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "convert_weights.py"))
    cw = importlib.util.module_from_spec(spec); spec.loader.exec_module(cw)
    sd = {"model." + k: torch.from_numpy(v) for k, v in st.items()}
    assert cw.convert({"model": None, "state_dict": sd, "metadata": {"input_shape": (80, 80, 1), "num_classes": c, "model_type": "v118_3"}})[0] == blob


# ---- (a) parity in every mode ------------------------------------------------------------------------------------------------------------

def test_float32_oracle_meets_the_arg_max_condition_on_the_test_set():
    """host only: with the fp32 oracle standing in for the device, the test set stays within the 1 % cap of the arg-max condition and the
    arg-max agrees wherever it is decided -- the condition is one an honest fp32 evaluation meets"""
    crops, p64, l64, l32, e32 = parity_set()
    n = identity_synth.N_TEST
    decided = top_two_gap(l64[:n]) > 2 * LOGIT_FACTOR * e32
    print(f"fp32 oracle on the test set: undecided {int((~decided).sum())} of {n} at gap <= {2 * LOGIT_FACTOR * e32:.3g}")
    assert (~decided).mean() <= UNDECIDED_CAP
    assert np.array_equal(l32[:n].argmax(1)[decided], l64[:n].argmax(1)[decided])


@pytest.mark.parametrize("mode,name", MODES)
def test_trained_net_equals_the_float64_oracle(mode, name):
    """Softmax within 1e-4, rows sum to 1 within 1e-5, all finite; logits within 8 x e32 (FP32, BF16X6, FP16X3; BF16X3 is reported, as in
    test_precision_modes_error_ladder); arg-max equal wherever the float64 top-two gap exceeds 2 x 8 x e32, at most 1 % left out.
    Measured (MI355X): see DESIGN.md section 4."""
    crops, p64, l64, l32, e32 = parity_set()
    blob, _ = trained_net.trained_blob()
    seg = make_net(blob)
    seg.set_identity_precision(mode)
    probs, logits = device_forward(seg, crops)
    if mode == capi.CNN_FP16X3:
        print("fp16x3 guard on the parity set (rerun, whole):", seg.guard_stats())
    seg.close()
    check_rows(name, probs, logits, p64, l64, e32, hold_logits=mode != capi.CNN_BF16X3)


# ---- (b) the range guard on real activations ---------------------------------------------------------------------------------------------

N_STEP = 25600              # one bench step's worth of crops


def classify(maxima):
    """-> (must_trip, must_not_trip, undecided) boolean arrays from the three per-stage maxima"""
    above = np.zeros(len(maxima[0]), bool)
    below = np.ones(len(maxima[0]), bool)
    for m, lim in zip(maxima, LIMITS):
        above |= ~(m <= lim * (1 + BAND))          # (a NaN is out of range as well)
        below &= m < lim * (1 - BAND)
    return above, below, ~above & ~below


@functools.lru_cache(maxsize=None)
def step_batch():
    """25600 crops (the test set tiled with fresh pose seeds) and their fp32 stage maxima on the trained net"""
    trained_net.assert_trained()
    st, _ = trained_net.trained_state()
    crops, _ = trained_net.identities().tiled_set(N_STEP)
    return crops, trained_net.stage_maxima(st, crops)


def guard_case(tag, st, crops, maxima):
    must, mustnot, und = classify(maxima)
    n, n_must, n_und = len(crops), int(must.sum()), int(und.sum())
    q = [np.quantile(m[np.isfinite(m)], [0.5, 0.99, 1.0]) for m in maxima]
    print(f"{tag}: {n} crops, stage maxima 50 / 99 / 100 %: " + "; ".join("%.4g / %.4g / %.4g" % tuple(v) for v in q) +
          f"; must-trip {n_must} ({100.0 * n_must / n:.3g} %), undecided {n_und}")
    assert n_und <= UNDECIDED_CAP * n, (tag, n_und)
    seg = make_net(weights.pack_blob(st, trained_net.CLASSES))
    seg.set_identity_precision(capi.CNN_FP16X3)
    probs, logits = device_forward(seg, crops)
    rerun, whole = seg.guard_stats()
    print(f"{tag}: guard_stats = ({rerun}, {whole}): trip rate {100.0 * rerun / n:.3g} % of the crops")
    bound = 3 * (n_must + n_und)
    if n_must == 0 and n_und == 0:
        assert (rerun, whole) == (0, False), (tag, rerun, whole)
    elif whole:
        assert bound > FB_MAX, (tag, rerun, whole, bound)
    else:
        assert n_must <= rerun <= bound, (tag, rerun, n_must, n_und)
    assert np.all(np.isfinite(probs))
    # every must-trip row meets the bars of (a), with e32 measured on those rows
    if n_must:
        idx = np.flatnonzero(must)
        idx = idx[np.linspace(0, len(idx) - 1, min(len(idx), 1024)).astype(np.int64)]     # (all of them up to 1024; evenly spread beyond that)
        p64, l64 = trained_net.oracle_f64(st, crops[idx])
        e32 = float(np.abs(trained_net.oracle_f32_logits(st, crops[idx]) - l64).max())
        check_rows(tag + " must-trip rows", probs[idx], logits[idx], p64, l64, e32, cap=False)
    # every row the guard did not touch has the bits it has in a batch of must-not-trip crops only.  A flag names the first and the last crop of
    # a pass, so the direct neighbours of a crop that may trip may be re-run with it; they keep their answer to 1e-5 either way
    if n_must or n_und:
        loud = must | und
        quiet = crops.copy()
        quiet[loud] = crops[np.flatnonzero(mustnot)[0]]
        qp, _ = device_forward(seg, quiet)
        assert seg.guard_stats() == (0, False), tag
        near = loud.copy(); near[1:] |= loud[:-1]; near[:-1] |= loud[1:]
        if not whole:
            assert probs[~near].tobytes() == qp[~near].tobytes(), tag
        nb = near & ~loud
        assert np.abs(probs[nb] - qp[nb]).max(initial=0.0) <= 1e-5, tag
    seg.close()
    return n_must, rerun, whole


def test_range_guard_on_a_bench_steps_worth_of_real_crops():
    """The natural trip rate of the fp16 range guard on a trained network (the number nobody had measured), and that the guard does what the
    float-oracle's stage maxima say it must.  Measured: see DESIGN.md section 4."""
    st, _ = trained_net.trained_state()
    crops, maxima = step_batch()
    guard_case("natural", st, crops, maxima)


def unseen_batch():
    st, _ = trained_net.trained_state()
    crops, maxima = step_batch()
    crops, maxima = crops.copy(), [m.copy() for m in maxima]
    extra = identity_synth.unseen_crops()
    rng = np.random.default_rng(17)
    # each pattern a few times: alone, next to another one, first and last crop of the batch
    pos = np.concatenate([[0, 1, N_STEP - 1], rng.choice(np.arange(2, N_STEP - 1), 8 * len(extra) - 3, replace=False)])
    put = np.tile(extra, (8, 1, 1, 1))
    crops[pos] = put
    for k, m in enumerate(trained_net.stage_maxima(st, put)):
        maxima[k][pos] = m
    return st, crops, maxima


def test_range_guard_with_crops_the_trained_statistics_never_saw():
    """saturated full frames and 255 / 0 checkerboards (periods 1, 2, 5) mixed into the batch; the stage maxima decide whether they trip"""
    st, crops, maxima = unseen_batch()
    guard_case("unseen", st, crops, maxima)


def test_range_guard_per_crop_rerun_with_a_realistic_spread_of_activations():
    """bn1's affine scaled (and bn2's running variance by the square, which takes the scale back out) so that about 0.5 % of the step's crops
    cross 4368 behind conv1: the per-crop re-run on a trained network's spread of activations instead of one loud crop among quiet ones
    (test_range_guard_is_per_crop).  The factor comes from the float64 maxima of the test set."""
    st, _ = trained_net.trained_state()
    crops, maxima = step_batch()
    x, _, _, _ = trained_net.held_out_reference()
    m64 = trained_net.stage_maxima(st, x, dtype=torch.float64)[0]
    f = np.float32(LIMITS[0] / np.quantile(m64, 0.995))
    st = {k: v.copy() for k, v in st.items()}
    st["bn1.weight"] = st["bn1.weight"] * f; st["bn1.bias"] = st["bn1.bias"] * f
    st["bn2.running_var"] = st["bn2.running_var"] * f * f
    n_must, rerun, whole = guard_case(f"scaled x{float(f):.4g}", st, crops, trained_net.stage_maxima(st, crops))
    assert n_must > 0 and not whole and rerun > 0


# ---- (c) the call shapes the tracker makes -----------------------------------------------------------------------------------------------

def test_small_calls_give_the_rows_of_the_large_call_on_the_trained_net():
    trained_net.assert_trained()
    blob, _ = trained_net.trained_blob()
    crops = trained_net.identities().test_set()[0][:1100]
    seg = make_net(blob)
    seg.set_identity_precision(capi.CNN_FP16X3)
    big = seg.probabilities(crops)
    for n in (1, 100, 1000, 1024):
        assert seg.probabilities(crops[:n]).tobytes() == big[:n].tobytes(), n
    seg.close()


def test_replayed_100_crop_call_reproduces_the_first_call():
    """ten consecutive 100-crop identify_device calls on the same buffers (direct launches, the capture, then replays of the captured graph),
    the crops rewritten in place with the same values before each: every call gives the first call's bits, and those are the oracle's rows"""
    trained_net.assert_trained()
    blob, _ = trained_net.trained_blob()
    x, _, p64, _ = trained_net.held_out_reference()
    src = torch.from_numpy(np.ascontiguousarray(x[:100, :, :, 0])).cuda()
    seg = make_net(blob)
    crops = torch.zeros_like(src)
    probs = torch.zeros((100, trained_net.CLASSES), dtype=torch.float32, device="cuda")
    first = None
    for rep in range(10):
        crops.copy_(src)
        probs.zero_()
        seg.identify_device(crops.data_ptr(), 100, probs.data_ptr())
        seg.synchronize()
        got = probs.cpu().numpy()
        if first is None:
            first = got
            assert np.abs(first - p64[:100]).max() <= 1e-4
        assert got.tobytes() == first.tobytes(), rep
    seg.close()


# ---- (d) the trainer's own forward -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def validation_reference():
    trained_net.assert_trained()
    st, _ = trained_net.trained_state()
    vx, vy = trained_net.identities().validation_set()
    _, l64 = trained_net.oracle_f64(st, vx)
    return vx, vy, l64, float(np.abs(trained_net.oracle_f32_logits(st, vx) - l64).max())


@pytest.mark.parametrize("precision", [0, 1])
def test_trainer_evaluate_on_the_trained_weights_equals_the_float64_oracle(precision):
    """Trainer.evaluate after the full run (a trainer created on the trained weights, at either precision) on the validation set: the float64
    oracle's cross entropy within 5e-5 x max(1, |loss|) per batch, and its correct count -- up to the samples whose float64 top-two gap is
    below the arg-max condition of (a), of which there may be 1 % at most"""
    blob, _ = trained_net.trained_blob()
    vx, vy, l64, e32 = validation_reference()
    z = l64 - l64.max(1, keepdims=True)
    ce = np.log(np.exp(z).sum(1)) - z[np.arange(len(vy)), vy]
    hit = l64.argmax(1) == vy
    loose = top_two_gap(l64) <= 2 * LOGIT_FACTOR * e32
    assert loose.mean() <= UNDECIDED_CAP, float(loose.mean())
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    B = identity_synth.BATCH
    tr = capi.Trainer(seg, blob, max_batch=B, lr=trained_net.LR, precision=precision)
    worst = 0.0
    for lo in range(0, len(vy), B):
        s = slice(lo, lo + B)
        loss, correct = tr.evaluate(vx[s].astype(np.float32), vy[s])
        ref = float(ce[s].mean())
        worst = max(worst, abs(loss - ref) / max(1.0, abs(ref)))
        assert abs(loss - ref) <= 5e-5 * max(1.0, abs(ref)), (lo, loss, ref)
        assert abs(correct - int(hit[s].sum())) <= int(loose[s].sum()), (lo, correct, int(hit[s].sum()), int(loose[s].sum()))
    print(f"precision {precision}: validation cross entropy {float(ce.mean()):.5f}, worst batch error {worst:.3g} (bar 5e-5), correct {int(hit.sum())} of {len(vy)}, loose {int(loose.sum())}")
    assert tr.export() == blob
    tr.close(); seg.close()
