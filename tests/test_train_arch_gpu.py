"""The training step of the identity networks v100 and v110 (trex_amd/csrc/train_arch.hip) against the float64 restatement
(tests/train_arch_ref.py, dtype=torch.float64) with injected dropout masks, at the cases of tests/train_arch_cases.py -- the smallest shapes at
which each new path can go wrong; what each reaches, and that the float32 restatement stays five times inside every bar of float64 at every one of
them, is shown on the CPU by test_train_arch_ref.py -- so a miss here is the device's.

The bars are test_train_gpu.py's and test_train_tiles_gpu.py's, taken against float64: loss 5e-5 max(1, |loss64|), `correct` equal, every element
of every gradient tensor within GRAD_RTOL = 2e-4 of max|g64| of its tensor (a bias in front of a BatchNorm -- v110's three conv biases and
fc1.bias -- has the true gradient 0 and is held to 1e-4 max(1, max|g64 of the matching weight|)), running statistics (bn4's included) and
parameters 1e-4 max(1, max|ref|), probabilities 1e-4.

  1. every case, both versions: one step against float64; the device's error per tensor is printed as a multiple of the float32 restatement's own
  2. three steps with Adam (21 x 13, 44 x 28): parameters, the step count, torch's shapes, the moments after the first step against the device's own
     gradient, and the parameters against Adam replayed on the host from the device's own gradients
  3. the export after those steps: the version in the header, trexhip_load_weights on a fresh context, identify / predict_device / the float64
     eval restatement in chunks, evaluate at n and at n = 1
  4. a second trainer gives the same bits (100 x 60, 14 x 100)
  5. a second step at a smaller batch on the same trainer (14 x 100, n = 5 then 3)
  6. trexhip_train_params.dropout is not read: the rates are the architecture's
  7. refusals: v110 at n = 1, a mask buffer of V118_3's size, v119 and v200, and a V118_3 trainer beside them
  8. one epoch of train_resident with ResidentLoader and ResidentValidation on a v110 trainer

Measured on the MI355X.  The device's error as a multiple of the float32 restatement's error against float64, worst tensor per case in the table's
order (no bar is set on it): v100 3.3, 17.4 (9 x 8, fc2.bias: 1e-6, the restatement happens to be within 1e-7 there), 6.9, 0.5, 0.2, 1.3, 1.1, 7.0;
v110 3.6, 4.1, 2.1, 1.4, 1.1, 1.1, 1.0, 1.3.  The worst gradient error itself is 0.195 of its bar (v110, conv1.weight at 80 x 80: 5.6e-4 against
2e-4 max|g64| = 2.9e-3) and 0.036 of it for v100; losses within 3.5e-6 relative; running statistics and the parameters after three steps within
6.1e-5; predict_device, identify on the exported blob and the float64 eval restatement within 7.5e-6 of each other."""
import functools
import numpy as np
import pytest
import torch

from trex_amd import capi, train_loop, weights
from oracle import cnn_train_oracle as tro
import train_arch_cases as tc
import train_arch_ref as ref
import uniqueness_ref as U

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4
BOTH = [(c, a) for c in tc.CASES for a in tc.ARCHS]
BOTH_IDS = [f"{tc.case_id(c)}-{a}" for c, a in BOTH]


def make_seg():
    p = capi.default_params(64, 64)
    p.max_batch = 1
    return capi.Segmenter(p)


def tensors(case, arch):
    W, H, ch, n, classes = case[0]
    return weights.shapes(classes, ch, W, H, arch)


def new_trainer(seg, case, arch, state=None, max_batch=None, lr=tc.LR, **kw):
    W, H, ch, n, classes = case[0]
    blob = weights.pack_blob(state if state is not None else tc.initial_state(case, arch), classes, ch, W, H, arch)
    tr = capi.Trainer(seg, blob, max_batch=max_batch or n, lr=lr, **kw)
    assert (tr.width, tr.height, tr.channels, tr.classes, tr.version) == (W, H, ch, classes, weights.ARCH_IDS[arch])
    assert tr.mask_row == 280
    return tr


def read_all(tr, case, arch, kind):
    return {nm: tr.read(i, kind, shp) for i, (nm, shp) in enumerate(tensors(case, arch))}


def step(tr, x, y, masks):
    dx = torch.from_numpy(x).cuda()
    dy = torch.from_numpy(y.astype(np.int32)).cuda()
    dm = torch.from_numpy(ref.pack_masks(masks)).cuda()
    out = tr.step_device(dx.data_ptr(), dy.data_ptr(), x.shape[0], dm.data_ptr())
    torch.cuda.synchronize()
    return out


def predict(tr, crops, classes):
    d = torch.from_numpy(crops).cuda()
    out = torch.full((len(crops), classes), -1.0, dtype=torch.float32, device="cuda")
    tr.predict_device(d.data_ptr(), len(crops), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def one_step(seg, case, arch, **kw):
    """a fresh trainer's first step on the case's inputs -> (loss, correct, gradients, parameters, the trainer)"""
    tr = new_trainer(seg, case, arch, **kw)
    loss, correct = step(tr, *tc.inputs(case, arch))
    return loss, correct, read_all(tr, case, arch, 1), read_all(tr, case, arch, 0), tr


def check_step(tag, loss, correct, ref_loss, ref_correct):
    print(f"{tag}: loss {loss!r} ref {ref_loss!r} correct {correct} ref {ref_correct}")
    assert abs(loss - ref_loss) <= 5e-5 * max(1.0, abs(ref_loss)), (tag, loss, ref_loss)
    assert correct == ref_correct, (tag, correct, ref_correct)


def hold_gradients(tag, arch, g, g64, own=None):
    """every element of every gradient tensor within the bar of float64; with `own` (the float32 restatement's gradients) the device's error is
    printed as a multiple of own's.  -> the worst such multiple and its tensor"""
    zero = ref.zero_gradient(arch)
    failed, worst = [], (0.0, None)
    for k in ref.trainable(arch):
        r = np.asarray(g64[k], np.float64)
        assert g[k].shape == r.shape and np.all(np.isfinite(g[k])), k
        if k in zero:
            err, tol = float(np.abs(g[k]).max()), 1e-4 * max(float(np.abs(g64[zero[k]]).max()), 1.0)
            e32 = float(np.abs(own[k]).max()) if own else None
        else:
            err, tol = float(np.abs(g[k] - r).max()), tc.GRAD_RTOL * float(np.abs(r).max())
            e32 = float(np.abs(own[k] - r).max()) if own else None
        line = f"{tag} grad {k}: err {err:.3g} tol {tol:.3g} = {err / tol:.3g} of the bar"
        if own:
            mult = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
            line += f" = {mult:.3g} x the float32 restatement's {e32:.3g}"
            if k not in zero and mult > worst[0]:
                worst = (mult, k)
        print(line)
        if not err <= tol:
            failed.append((k, err, tol))
    assert not failed, (tag, failed)
    return worst


def hold_statistics(tag, arch, p, stats64):
    for k in ref.buffers(arch):
        err = float(np.abs(p[k] - stats64[k]).max())
        print(f"{tag} {k}: err {err:.3g}")
        assert err <= 1e-4 * max(1.0, float(np.abs(stats64[k]).max())), (tag, k, err)


# ---- 1. one step of every case against float64 ----
@pytest.mark.parametrize("case,arch", BOTH, ids=BOTH_IDS)
def test_one_step_against_float64(case, arch):
    both = tc.restatements(case, arch)
    _, _, g32, _ = both[torch.float32]
    loss64, correct64, g64, stats64 = both[torch.float64]
    seg = make_seg()
    loss, correct, g, p, tr = one_step(seg, case, arch)
    assert tr.steps == 1
    tr.close()
    seg.close()
    tag = f"{tc.case_id(case)} {arch}"
    check_step(tag, loss, correct, loss64, correct64)
    mult, where = hold_gradients(tag, arch, g, g64, own=g32)
    print(f"{tag}: worst multiple of the float32 restatement's error {mult:.3g} ({where})")
    hold_statistics(tag, arch, p, stats64)
    assert (arch == "v110") == ("bn4.running_var" in stats64)


# ---- 2. and 3. three steps with Adam, the export behind them ----
@functools.lru_cache(maxsize=None)
def chain(W, H, arch):
    """three steps on the device and by the float64 restatement, then everything tests 2 and 3 look at, computed once"""
    case = tc.find(W, H)
    _, _, ch, n, classes = case[0]
    state = tc.initial_state(case, arch)
    adam64, adam_dev = ref.new_adam_state(arch, state), ref.new_adam_state(arch, state)
    cur64 = replay = state
    seg = make_seg()
    tr = new_trainer(seg, case, arch)
    out = {"case": case, "n_tensors": len(tensors(case, arch))}
    for s in range(3):
        x, y, masks = tc.inputs(case, arch, s)
        cur64 = ref.train_step(arch, cur64, adam64, x, y, masks, tc.LR, dtype=torch.float64)[0]
        # the step's loss has its reference in the float64 restatement of this one step from what the device itself holds in front of it: the two
        # chains' parameters part by Adam's +-lr on rounding noise, and v100's unnormalised loss moves by 6e-4 on that (the float32 restatement's
        # own chain is that far from the float64 one at 44 x 28)
        loss64, correct64 = ref.forward_backward(arch, read_all(tr, case, arch, 0), x, y, masks, dtype=torch.float64, threads=16)[:2]
        loss, correct = step(tr, x, y, masks)
        g = read_all(tr, case, arch, 1)
        replay = ref.adam_update(arch, replay, adam_dev, {k: g[k] for k in ref.trainable(arch)}, tc.LR)
        if s == 0:
            out["first"] = (g, read_all(tr, case, arch, 2), read_all(tr, case, arch, 3))
        out[f"step{s}"] = (loss, correct, loss64, correct64)
    out["steps"] = tr.steps
    out["final"], out["final64"], out["replay"] = read_all(tr, case, arch, 0), cur64, replay
    with pytest.raises(capi.TrexHipError) as e:                       # torch's shapes: conv3 has 100 channels, never the padded 128
        tr.read([nm for nm, _ in tensors(case, arch)].index("conv3.weight"), 0, (128, 64, 5, 5))
    out["read128"] = e.value.code
    out["blob"] = tr.export()
    crops = tc.crops(case, 16, 77)
    out["crops"] = crops
    out["predict"] = predict(tr, crops, classes)                     # max_batch = n < 16: chunks
    x, y, _ = tc.inputs(case, arch, 5)
    out["eval_in"] = (x, y)
    out["eval"] = tr.evaluate(x, y)
    out["eval1"] = tr.evaluate(x[:1], y[:1])
    assert tr.steps == 3
    tr.close()
    seg.close()
    fresh = make_seg()
    fresh.load_weights(out["blob"])
    out["loaded_version"], out["loaded_size"] = fresh.network_version(), fresh.network_image_size()
    out["identify"] = fresh.probabilities(crops)
    fresh.close()
    return out


CHAINS = [(21, 13, "v100"), (44, 28, "v100"), (21, 13, "v110"), (44, 28, "v110")]


@pytest.mark.parametrize("W,H,arch", CHAINS)
def test_three_steps_with_adam_against_float64(W, H, arch):
    c = chain(W, H, arch)
    tag = f"{W}x{H} {arch}"
    for s in range(3):
        loss, correct, loss64, correct64 = c[f"step{s}"]
        check_step(f"{tag} step {s}", loss, correct, loss64, correct64)
    assert c["steps"] == 3 and c["read128"] == E_INVALID
    assert c["n_tensors"] == (10 if arch == "v100" else 26)
    for k, shp in tensors(c["case"], arch):
        r = c["final64"][k]
        assert c["final"][k].shape == tuple(shp) == r.shape, k
        err = float(np.abs(c["final"][k] - r).max())
        print(f"{tag} final {k}: err {err:.3g}")
        assert err <= 1e-4 * max(1.0, float(np.abs(r).max())), (k, err)
    # the optimizer itself: the parameters are Adam's (oracle.cnn_train_oracle.adam_update, fp32) on the device's own gradients, to a few ulp
    for k in ref.trainable(arch):
        r = c["replay"][k]
        err = float(np.abs(c["final"][k] - r).max())
        assert err <= 1e-6 * max(1.0, float(np.abs(r).max())), ("replay", k, err)
        assert np.any(c["final"][k] != tc.initial_state(c["case"], arch)[k]), k
    # the moments start at 0: after one step m = (1 - beta1) g and v = (1 - beta2) g g of the device's own gradient (test_train_tiles_gpu.py, 3.)
    beta1, beta2 = float(np.float32(0.9)), float(np.float32(0.999))
    g, m, v = c["first"]
    for k in ref.trainable(arch):
        g64 = g[k].astype(np.float64)
        assert np.any(g64 != 0), k
        for what, got, want in (("m", m[k], (1.0 - beta1) * g64), ("v", v[k], (1.0 - beta2) * g64 * g64)):
            zero = g64 == 0
            assert np.all(got[zero] == 0), (what, k)
            tiny = np.abs(want) < 2e-38
            rel = np.abs(got[~tiny] - want[~tiny]) / np.abs(want[~tiny])
            assert np.all(rel <= 1e-6), (what, k, float(rel.max()))
            assert np.all(np.abs(got[tiny] - want[tiny]) <= 2e-38), (what, k)
    for k in ref.buffers(arch):
        assert not m[k].any() and not v[k].any(), k


@pytest.mark.parametrize("W,H,arch", CHAINS)
def test_the_export_loads_and_predicts(W, H, arch):
    c = chain(W, H, arch)
    case = c["case"]
    _, _, ch, n, classes = case[0]
    blob = c["blob"]
    assert weights.blob_arch(blob) == arch and c["loaded_version"] == weights.ARCH_IDS[arch] and c["loaded_size"] == (W, H)
    st, c2, ch2 = weights.unpack_blob(blob, arch)
    assert (c2, ch2) == (classes, ch)
    for k in st:
        assert st[k].tobytes() == c["final"][k].tobytes(), k          # the blob is the trainer's parameters, bit for bit
    want = ref.predict(arch, st, c["crops"], dtype=torch.float64)
    e_tr, e_id = float(np.abs(c["predict"] - want).max()), float(np.abs(c["identify"] - want).max())
    print(f"{W}x{H} {arch}: max |dp| predict_device {e_tr:.3g}, identify {e_id:.3g}, between them {float(np.abs(c['predict'] - c['identify']).max()):.3g}")
    assert len(c["crops"]) > n and e_tr <= 1e-4 and e_id <= 1e-4 and np.abs(c["predict"] - c["identify"]).max() <= 1e-4
    x, y = c["eval_in"]
    for got, (xx, yy) in ((c["eval"], (x, y)), (c["eval1"], (x[:1], y[:1]))):
        loss64, correct64, _ = ref.evaluate(arch, st, xx, yy, dtype=torch.float64)
        check_step(f"{W}x{H} {arch} evaluate n = {len(yy)}", got[0], got[1], loss64, correct64)


# ---- 4. determinism ----
@pytest.mark.parametrize("arch", tc.ARCHS)
@pytest.mark.parametrize("W,H", [(100, 60), (14, 100)])
def test_a_second_trainer_gives_the_same_bits(W, H, arch):
    case = tc.find(W, H)
    seg = make_seg()
    runs = []
    for _ in range(2):
        loss, correct, g, p, tr = one_step(seg, case, arch)
        tr.close()
        runs.append((loss, correct, g, p))
    seg.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k, _ in tensors(case, arch):
        assert runs[0][2][k].tobytes() == runs[1][2][k].tobytes(), ("gradient", k)
        assert runs[0][3][k].tobytes() == runs[1][3][k].tobytes(), ("parameter", k)


# ---- 5. a smaller batch behind a larger one ----
@pytest.mark.parametrize("arch", tc.ARCHS)
def test_a_second_step_at_a_smaller_batch(arch):
    """n = 5 and then n = 3 on the same trainer at 14 x 100: nothing of the first batch is left in a sum.  Each step against the float64 restatement
    of that one step from the parameters and statistics the device itself holds in front of it"""
    case = tc.find(14, 100)
    assert case[0][3] == 5
    seg = make_seg()
    tr = new_trainer(seg, case, arch)
    for s, n in enumerate((5, 3)):
        x, y, masks = tc.inputs(case, arch, s, n=n)
        held = read_all(tr, case, arch, 0)
        loss, correct = step(tr, x, y, masks)
        g, p = read_all(tr, case, arch, 1), read_all(tr, case, arch, 0)
        loss64, correct64, g64, stats64 = ref.forward_backward(arch, held, x, y, masks, dtype=torch.float64, threads=16)
        tag = f"14x100 {arch} step {s} (n = {n})"
        check_step(tag, loss, correct, loss64, correct64)
        hold_gradients(tag, arch, g, g64)
        hold_statistics(tag, arch, p, stats64)
    assert tr.steps == 2
    tr.close()
    seg.close()


# ---- 6. the rates are the architecture's ----
def test_the_dropout_parameter_is_not_read():
    case = tc.find(21, 13)
    seg = make_seg()
    runs = []
    for rate in (0.05, 0.9):
        loss, correct, g, p, tr = one_step(seg, case, "v100", dropout=rate)
        tr.close()
        runs.append((loss, correct, g, p))
    seg.close()
    assert runs[0][:2] == runs[1][:2]
    for k, _ in tensors(case, "v100"):
        assert runs[0][2][k].tobytes() == runs[1][2][k].tobytes() and runs[0][3][k].tobytes() == runs[1][3][k].tobytes(), k


# ---- 7. refusals ----
def test_refusals():
    case = tc.find(9, 8)
    W, H, ch, n, classes = case[0]
    seg = make_seg()
    tr = new_trainer(seg, case, "v110")
    x, y, masks = tc.inputs(case, "v110")
    before = read_all(tr, case, "v110", 0)
    for call in (lambda: step(tr, x[:1], y[:1], {k: m[:1] for k, m in masks.items()}), lambda: tr.step(x[:1], y[:1])):
        with pytest.raises(capi.TrexHipError) as e:
            call()
        assert e.value.code == E_INVALID and "v110" in str(e.value), str(e.value)
    assert tr.steps == 0
    after = read_all(tr, case, "v110", 0)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert np.isfinite(tr.evaluate(x[:1], y[:1])[0]) and predict(tr, tc.crops(case, 1, 3), classes).shape == (1, classes)      # eval and predict take n = 1
    with pytest.raises(ValueError, match="280"):                       # a mask buffer of V118_3's size on the host route
        tr.step(x, y, np.ones(n * 308, np.uint8))
    loss, correct = tr.step(x, y, ref.pack_masks(masks))              # ... and the right one runs
    both = tc.restatements(case, "v110")[torch.float64]
    check_step("9x8 v110 host route", loss, correct, both[0], both[1])
    assert tr.steps == 1
    tr.close()
    for arch, size in (("v119", 16), ("v200", 27)):
        blob = weights.pack_blob(weights.synthetic_state(5, 3, 1, size, size, arch), 5, 1, size, size, arch)
        with pytest.raises(capi.TrexHipError) as e:
            capi.Trainer(seg, blob, max_batch=4)
        assert e.value.code == E_UNSUPPORTED and arch in str(e.value) and "trexhip_trainer_create" in str(e.value), str(e.value)
    # a V118_3 trainer on the same context is what it was: its own mask row, its 24 tensors, a step that runs
    st = weights.synthetic_state(5, 9, 1, 16, 16)
    old = capi.Trainer(seg, weights.pack_blob(st, 5, 1, 16, 16), max_batch=4, lr=1e-3)
    assert old.version == 0 and old.mask_row == 308
    xs = tc.textured(4, 5, 1, 16, 16)
    ys = np.arange(4, dtype=np.int32)
    loss, _ = old.step(xs, ys, np.ones(4 * 308, np.uint8))
    ones = {"d1": np.ones((4, 16), bool), "d2": np.ones((4, 64), bool), "d3": np.ones((4, 128), bool), "d4": np.ones((4, 100), bool)}
    want = tro.forward_backward(st, xs, ys, ones, threads=16, dtype=torch.float64)[0]
    assert abs(loss - want) <= 5e-5 * max(1.0, abs(want)) and old.steps == 1 and old.read(23, 0, (5,)).shape == (5,)
    old.close()
    seg.close()


# ---- 8. the resident path ----
def test_one_resident_epoch_on_a_v110_trainer():
    W = H = 16
    classes, ch, batch = 4, 1, 8
    case = ((W, H, ch, batch, classes), 4100, "resident")
    seg = make_seg()
    tr = new_trainer(seg, case, "v110", lr=1e-3)
    pool = tc.crops(case, 24, 11)
    y = (np.arange(24) % classes).astype(np.int32)
    train = train_loop.ResidentLoader(seg, pool, y, batch_size=batch, seed=2)
    val = train_loop.ResidentLoader(seg, pool[:16], y[:16], batch_size=batch, augment=False, shuffle=False)
    rv = train_loop.ResidentValidation(tr, seg, pool, y)
    hist = train_loop.train_resident(tr, train, val, rv, None, {"epochs": 1})
    assert len(hist) == 1 and tr.steps == 3
    acc = rv.per_class_accuracy()
    rows = predict(tr, pool, classes)
    assert np.all(np.isfinite(rows)) and np.abs(rows.sum(1) - 1).max() <= 1e-5
    assert acc.shape == (classes,) and np.array_equal(acc, U.per_class_accuracy(rows, y, classes))
    train.close(); val.close(); rv.close(); tr.close()
    seg.close()
