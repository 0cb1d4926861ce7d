"""The training step of the category network (ChainTrainer in trex_amd/csrc/train_arch.hip: train_any.hip's chain at 3 taps with a normalising conv1 pair and
element-wise dropout masks) against the float64 restatement (tests/category_train_ref.py, dtype=torch.float64) with injected masks, at the cases of
tests/category_train_cases.py -- the smallest shapes at which each path can go wrong; that the float32 restatement stays five times inside every
bar of float64 at every one of them is shown on the CPU by test_category_train_ref.py, so a miss here is the device's.

The bars are the project's own (train_arch_cases.py), taken against float64: loss 5e-5 max(1, |loss64|), `correct` equal, every element of every
gradient tensor within GRAD_RTOL = 2e-4 of max|g64| of its tensor (a convolution bias stands in front of a BatchNorm, has the true gradient 0 and is
held to 1e-4 max(1, max|g64 of the matching weight|)), running statistics and parameters 1e-4 max(1, max|ref|), probabilities 1e-4.

  1. every case: one step against float64; the device's error per tensor is printed as a multiple of the float32 restatement's own
  2. three chained steps at lr 1e-5 (21 x 13, 24 x 16 at n = 1): parameters and Adam moments against float64, then the evaluation
  3. predict_device on uint8 crops, trexhip_categorize_device on the exported blob and the float64 eval restatement; the export round trip is exact
  4. the normalisation and the padding at 9 x 8 x 3: border pixels of byte 0, large border taps (the wrong first layers miss this check by orders
     of magnitude: test_category_train_ref.py)
  5. determinism: the same seed gives the same bytes with library-drawn masks, another seed gives other bytes
  6. trexhip_trainer_keep_mask_bytes for all three trainer types; a step with all-ones masks against float64
  7. refusals
  8. train_loop.train_category against the CPU restatement's run with the same index lists and masks

Measured on the MI355X.  The device's error as a multiple of the float32 restatement's error against float64, worst tensor per case in the table's
order (no bar is set on it): 1.9, 2.0, 2.0, 1.5, 0.7, 2.9, 3.2, 1.3, 1.6.  The worst gradient error itself is 0.0105 of its bar (100 x 14,
batch_norm2.bias: 5.7e-7 against 5.4e-5); parameters after three steps within 2.8e-5 (a convolution bias in front of a BatchNorm: Adam's +-lr on
rounding noise; every other tensor within 2.9e-6); predict_device, categorize_device on the exported blob and the float64 eval restatement within
7.5e-8 of each other; train_category's ten epoch losses within 1.4e-6 of the restatement's run, its validation loss within 1.2e-5.  Which test
catches which mutation of the chain: profiles/train_category_mutants.txt."""
import functools
import numpy as np
import pytest
import torch

from trex_amd import capi, train_loop, weights
import category_train_cases as tc
import category_train_ref as ref
from test_category_train_ref import border_batch

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4


def make_seg():
    p = capi.default_params(64, 64)
    p.max_batch = 1
    return capi.Segmenter(p)


def blob_of(case, state=None):
    W, H, ch, n, categories = case[0]
    return weights.pack_category_blob(state if state is not None else tc.initial_state(case), categories, ch, W, H)


def new_trainer(seg, case, state=None, max_batch=None, lr=tc.LR, **kw):
    W, H, ch, n, categories = case[0]
    tr = capi.Trainer(seg, blob_of(case, state), max_batch=max_batch or n, lr=lr, **kw)
    assert (tr.width, tr.height, tr.channels, tr.classes, tr.version) == (W, H, ch, categories, capi.Trainer.NET_CATEGORY)
    assert tr.mask_row == ref.mask_bytes(1, W, H) and tr.keep_mask_bytes(n) == ref.mask_bytes(n, W, H)
    return tr


def read_all(tr, case, kind):
    return {nm: tr.read(i, kind, shp) for i, (nm, shp) in enumerate(tc.tensors(case))}


def step(tr, x, y, masks):
    dx = torch.from_numpy(x).cuda()
    dy = torch.from_numpy(y.astype(np.int32)).cuda()
    dm = torch.from_numpy(ref.pack_masks(masks)).cuda()
    out = tr.step_device(dx.data_ptr(), dy.data_ptr(), x.shape[0], dm.data_ptr())
    torch.cuda.synchronize()
    return out


def predict(tr, crops, categories):
    d = torch.from_numpy(crops).cuda()
    out = torch.full((len(crops), categories), -1.0, dtype=torch.float32, device="cuda")
    tr.predict_device(d.data_ptr(), len(crops), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_step(tag, loss, correct, ref_loss, ref_correct):
    print(f"{tag}: loss {loss!r} ref {ref_loss!r} correct {correct} ref {ref_correct}")
    assert abs(loss - ref_loss) <= 5e-5 * max(1.0, abs(ref_loss)), (tag, loss, ref_loss)
    assert correct == ref_correct, (tag, correct, ref_correct)


def hold_gradients(tag, g, g64, own=None):
    """every element of every gradient tensor within the bar of float64; with `own` (the float32 restatement's gradients) the device's error is
    printed as a multiple of own's.  -> the worst such multiple and its tensor"""
    failed, worst = [], (0.0, None)
    for k in ref.trainable():
        assert g[k].shape == g64[k].shape and np.all(np.isfinite(g[k])), k
        err, tol = tc.gradient_error(k, g, g64)
        line = f"{tag} grad {k}: err {err:.3g} tol {tol:.3g} = {err / tol:.3g} of the bar"
        if own:
            e32 = tc.gradient_error(k, own, g64)[0]
            mult = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
            line += f" = {mult:.3g} x the float32 restatement's {e32:.3g}"
            if k not in tc.ZERO_GRADIENT and mult > worst[0]:
                worst = (mult, k)
        print(line)
        if not err <= tol:
            failed.append((k, err, tol))
    assert not failed, (tag, failed)
    return worst


def hold_statistics(tag, p, stats64):
    for k in ref.buffers():
        err = float(np.abs(p[k] - stats64[k]).max())
        print(f"{tag} {k}: err {err:.3g}")
        assert err <= 1e-4 * max(1.0, float(np.abs(stats64[k]).max())), (tag, k, err)


# ---- 1. one step of every case against float64 ----
@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_one_step_against_float64(case):
    both = tc.restatements(case)
    _, _, g32, _ = both[torch.float32]
    loss64, correct64, g64, stats64 = both[torch.float64]
    seg = make_seg()
    tr = new_trainer(seg, case)
    loss, correct = step(tr, *tc.inputs(case))
    g, p = read_all(tr, case, 1), read_all(tr, case, 0)
    assert tr.steps == 1
    tr.close()
    seg.close()
    tag = tc.case_id(case)
    check_step(tag, loss, correct, loss64, correct64)
    mult, where = hold_gradients(tag, g, g64, own=g32)
    print(f"{tag}: worst multiple of the float32 restatement's error {mult:.3g} ({where})")
    hold_statistics(tag, p, stats64)


# ---- 2. and 3. three steps with Adam, the export behind them ----
@functools.lru_cache(maxsize=None)
def chain(W, H):
    """three steps on the device and by the float64 restatement, then everything tests 2 and 3 look at, computed once"""
    case = tc.find(W, H)
    _, _, ch, n, categories = case[0]
    c64 = ref.Chain(tc.initial_state(case), tc.LR, dtype=torch.float64)
    seg = make_seg()
    tr = new_trainer(seg, case)
    out = {"case": case}
    for s in range(3):
        x, y, masks = tc.inputs(case, s)
        c64.step(x, y, masks)
        # the step's loss has its reference in the float64 restatement of this one step from what the device itself holds in front of it
        loss64, correct64 = ref.forward_backward(read_all(tr, case, 0), x, y, masks, dtype=torch.float64, threads=16)[:2]
        loss, correct = step(tr, x, y, masks)
        out[f"step{s}"] = (loss, correct, loss64, correct64)
    out["steps"] = tr.steps
    out["final"], out["m"], out["v"] = read_all(tr, case, 0), read_all(tr, case, 2), read_all(tr, case, 3)
    out["final64"], (out["m64"], out["v64"]) = c64.state(), c64.moments()
    with pytest.raises(capi.TrexHipError) as e:                       # torch's shapes: conv3 has 100 channels, never the padded 128
        tr.read([nm for nm, _ in tc.tensors(case)].index("conv3.weight"), 0, (128, 64, 3, 3))
    out["read128"] = e.value.code
    out["blob"] = tr.export()
    crops = tc.crops(case, 16, 77)
    out["crops"] = crops
    out["predict"] = predict(tr, crops, categories)                  # max_batch = n < 16: chunks
    x, y, _ = tc.inputs(case, 5)
    out["eval_in"] = (x, y)
    out["eval"] = tr.evaluate(x, y)
    out["eval1"] = tr.evaluate(x[:1], y[:1])
    assert tr.steps == 3
    tr.close()
    # the exported blob: into the inference slot of a fresh context, and into a second trainer
    fresh = make_seg()
    fresh.load_category_weights(out["blob"])
    out["info"] = fresh.category_info()
    d = torch.from_numpy(crops).cuda()
    labels = torch.full((len(crops),), -1, dtype=torch.int32, device="cuda")
    probs = torch.full((len(crops), categories), -1.0, dtype=torch.float32, device="cuda")
    fresh.categorize_device(d.data_ptr(), len(crops), labels.data_ptr(), probs.data_ptr())
    torch.cuda.synchronize()
    out["cat_labels"], out["cat_probs"] = labels.cpu().numpy(), probs.cpu().numpy()
    again = capi.Trainer(fresh, out["blob"], max_batch=2)
    out["again"] = read_all(again, case, 0)
    out["blob_again"] = again.export()
    again.close()
    with pytest.raises(capi.TrexHipError, match="magic"):            # trexhip_load_weights keeps refusing category blobs
        fresh.load_weights(out["blob"])
    fresh.close()
    seg.close()
    return out


CHAINS = [(21, 13), (24, 16)]


@pytest.mark.parametrize("W,H", CHAINS)
def test_three_steps_with_adam_against_float64(W, H):
    c = chain(W, H)
    for s in range(3):
        loss, correct, loss64, correct64 = c[f"step{s}"]
        check_step(f"{W}x{H} step {s}", loss, correct, loss64, correct64)
    assert c["steps"] == 3 and c["read128"] == E_INVALID and len(tc.tensors(c["case"])) == 22
    initial = tc.initial_state(c["case"])
    for k, shp in tc.tensors(c["case"]):
        r = c["final64"][k]
        assert c["final"][k].shape == tuple(shp) == r.shape, k
        err = float(np.abs(c["final"][k] - r).max())
        print(f"{W}x{H} final {k}: err {err:.3g}")
        assert err <= 1e-4 * max(1.0, float(np.abs(r).max())), (k, err)
        assert np.any(c["final"][k] != initial[k]), k
    # Adam's moments: exp_avg within the gradients' bar (it is a mean of three gradients), exp_avg_sq within twice that relative to its largest element
    for k in ref.trainable():
        m64, v64 = c["m64"][k], c["v64"][k]
        scale = float(np.abs(c["m64"][tc.ZERO_GRADIENT[k]]).max()) if k in tc.ZERO_GRADIENT else float(np.abs(m64).max())
        tol = 1e-4 * max(1.0, scale) if k in tc.ZERO_GRADIENT else tc.GRAD_RTOL * scale
        em = float(np.abs(c["m"][k] - m64).max())
        print(f"{W}x{H} exp_avg {k}: err {em:.3g} tol {tol:.3g}")
        assert em <= tol, ("exp_avg", k, em, tol)
        if k not in tc.ZERO_GRADIENT:
            ev = float(np.abs(c["v"][k] - v64).max())
            assert ev <= 2 * tc.GRAD_RTOL * float(np.abs(v64).max()), ("exp_avg_sq", k, ev)
    for k in ref.buffers():
        assert not c["m"][k].any() and not c["v"][k].any(), k


@pytest.mark.parametrize("W,H", CHAINS)
def test_the_export_predicts_categorises_and_round_trips(W, H):
    c = chain(W, H)
    case = c["case"]
    _, _, ch, n, categories = case[0]
    blob = c["blob"]
    st, cats2, ch2, w2, h2 = weights.unpack_category_blob(blob)
    assert (cats2, ch2, w2, h2) == (categories, ch, W, H) == c["info"]
    for k in st:
        assert st[k].tobytes() == c["final"][k].tobytes(), k          # the blob is the trainer's parameters, bit for bit
        assert c["again"][k].tobytes() == st[k].tobytes(), k          # ... and a trainer created from it holds the same bits
    assert c["blob_again"] == blob
    want = ref.predict(st, c["crops"], dtype=torch.float64)
    e_tr, e_cat = float(np.abs(c["predict"] - want).max()), float(np.abs(c["cat_probs"] - want).max())
    between = float(np.abs(c["predict"] - c["cat_probs"]).max())
    print(f"{W}x{H}: max |dp| predict_device {e_tr:.3g}, categorize_device {e_cat:.3g}, between them {between:.3g}")
    assert len(c["crops"]) > n and e_tr <= 1e-4 and e_cat <= 1e-4 and between <= 1e-4
    assert np.array_equal(c["cat_labels"], want.argmax(1)) and np.array_equal(c["predict"].argmax(1), want.argmax(1))
    x, y = c["eval_in"]
    for got, (xx, yy) in ((c["eval"], (x, y)), (c["eval1"], (x[:1], y[:1]))):
        loss64, correct64, _ = ref.evaluate(st, xx, yy, dtype=torch.float64)
        check_step(f"{W}x{H} evaluate n = {len(yy)}", got[0], got[1], loss64, correct64)


# ---- 4. the normalisation and the padding ----
def test_the_first_layer_normalises_then_pads():
    case = tc.find(9, 8)
    st, x, y, masks = border_batch(case)
    loss64, correct64, g64, stats64 = ref.forward_backward(st, x, y, masks, dtype=torch.float64)
    seg = make_seg()
    tr = new_trainer(seg, case, state=st)
    loss, correct = step(tr, x, y, masks)
    g, p = read_all(tr, case, 1), read_all(tr, case, 0)
    tr.close()
    seg.close()
    check_step("9x8 border", loss, correct, loss64, correct64)
    hold_gradients("9x8 border", g, g64)
    hold_statistics("9x8 border", p, stats64)


# ---- 5. determinism ----
def run_drawn(seg, case, seed):
    tr = new_trainer(seg, case, seed=seed)
    for s in range(3):
        x, y, _ = tc.inputs(case, s)
        dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        tr.step_device(dx.data_ptr(), dy.data_ptr(), len(y), 0)
    blob = tr.export()
    tr.close()
    return blob


@pytest.mark.parametrize("W,H", [(100, 60), (14, 100)])
def test_the_same_seed_gives_the_same_bytes(W, H):
    case = tc.find(W, H)
    seg = make_seg()
    a, b, other = run_drawn(seg, case, 5), run_drawn(seg, case, 5), run_drawn(seg, case, 6)
    seg.close()
    assert a == b and a != other and a != blob_of(case)
    assert all(np.all(np.isfinite(v)) for v in weights.unpack_category_blob(a)[0].values())


# ---- 6. the mask sizes of the three trainer types; all-ones masks ----
def test_keep_mask_bytes_and_all_ones_masks():
    seg = make_seg()
    old = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(5, 9, 1, 16, 16), 5, 1, 16, 16), max_batch=4)
    arch = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(5, 9, 1, 16, 16, arch="v100"), 5, 1, 16, 16, arch="v100"), max_batch=4)
    assert [old.keep_mask_bytes(n) for n in (0, 1, 4)] == [0, 308, 1232] and [arch.keep_mask_bytes(n) for n in (0, 1, 4)] == [0, 280, 1120]
    assert old.mask_row == 308 and arch.mask_row == 280
    old.close(); arch.close()
    assert capi.lib().trexhip_trainer_keep_mask_bytes(None, 3) == 0
    case = tc.find(21, 13)
    W, H, ch, n, categories = case[0]
    tr = new_trainer(seg, case)
    assert tr.keep_mask_bytes(n) == n * (6 * 10 * 16 + 3 * 5 * 64 + 1 * 2 * 100 + 100) and tr.keep_mask_bytes(0) == 0
    x, y, _ = tc.inputs(case)
    ones = ref.ones_masks(n, W, H)
    with pytest.raises(ValueError, match=str(tr.mask_row)):             # a mask buffer of v100's size on the host route
        tr.step(x, y, np.ones(n * 280, np.uint8))
    loss, correct = tr.step(x, y, ref.pack_masks(ones))                 # ... and the right one runs
    g = read_all(tr, case, 1)
    tr.close()
    seg.close()
    loss64, correct64, g64, _ = ref.forward_backward(tc.initial_state(case), x, y, ones, dtype=torch.float64)
    check_step("21x13 all-ones masks, host route", loss, correct, loss64, correct64)
    hold_gradients("21x13 all-ones masks", g, g64)


# ---- 7. refusals ----
def test_refusals():
    case = tc.find(9, 8)
    W, H, ch, n, categories = case[0]
    good = blob_of(case)
    seg = make_seg()

    def hdr(**kw):
        h = np.frombuffer(good[:32], np.int32).copy()
        for k, v in kw.items():
            h[{"categories": 2, "width": 3, "height": 4, "channels": 5}[k]] = v
        return h.tobytes() + good[32:]

    for field, bad, code in (("size", good[:-4], E_INVALID), ("size", good[:20], E_INVALID), ("categories", hdr(categories=0), E_INVALID),
                             ("categories", hdr(categories=1025), E_INVALID), ("channels", hdr(channels=2), E_UNSUPPORTED),
                             ("width", hdr(width=7), E_UNSUPPORTED), ("height", hdr(height=257), E_UNSUPPORTED)):
        errors = []
        for call in (lambda: capi.Trainer(seg, bad, max_batch=4), lambda: seg.load_category_weights(bad)):      # the loader's codes and field names
            with pytest.raises(capi.TrexHipError, match=field) as e:
                call()
            assert e.value.code == code, (field, e.value.code)
            errors.append(str(e.value).split(": ", 2)[2])                 # behind "libtrexhip error <code>: <entry point>: "
        assert errors[0] == errors[1], errors
    # a target >= categories: the device's flag, parameters unchanged
    tr = new_trainer(seg, case)
    x, y, masks = tc.inputs(case)
    before = read_all(tr, case, 0)
    bad_y = y.copy()
    bad_y[1] = categories
    with pytest.raises(capi.TrexHipError, match="target") as e:
        step(tr, x, bad_y, masks)
    assert e.value.code == E_INVALID and tr.steps == 0
    after = read_all(tr, case, 0)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    loss, correct = step(tr, x, y, masks)                               # the trainer goes on
    both = tc.restatements(case)[torch.float64]
    check_step("9x8 after a refused step", loss, correct, both[0], both[1])
    assert tr.steps == 1
    tr.close()
    # an identity blob still gives an identity trainer
    for arch, version, row in ((None, 0, 308), ("v100", 1, 280)):
        kw = {"arch": arch} if arch else {}
        old = capi.Trainer(seg, weights.pack_blob(weights.synthetic_state(5, 9, 1, 16, 16, **kw), 5, 1, 16, 16, **kw), max_batch=4)
        assert old.version == version and old.mask_row == row
        old.close()
    seg.close()


# ---- 8. perform_training on the device ----
def squares(n, seed):
    """16 x 16 x 1 crops in two categories: a bright square on the left or on the right half, on a noisy dark background"""
    rng = np.random.default_rng(seed)
    y = (np.arange(n) % 2).astype(np.int32)
    x = rng.integers(0, 40, (n, 16, 16, 1)).astype(np.uint8)
    for i in range(n):
        r, c = rng.integers(2, 9), rng.integers(1, 3) + 8 * y[i]
        x[i, r:r + 5, c:c + 5, 0] = rng.integers(180, 255)
    return x, y


def test_train_category_follows_the_restatement():
    W = H = 16
    categories, epochs, batch, seed, lr = 2, 10, 32, 7, 1e-4     # the reference's epochs, batch and learning rate
    x, y = squares(144, 3)
    val = np.arange(96, 144)
    state = weights.synthetic_category_state(categories, 21, channels=1, width=W, height=H)
    blob = weights.pack_category_blob(state, categories, 1, W, H)
    masks = lambda e, b, n: ref.draw_masks(n, W, H, 1000 * e + b)
    seg = make_seg()
    hist = {}
    out = train_loop.train_category(seg, blob, x, y, val, seed=seed,
                                    keep_masks=lambda e, b, n: ref.pack_masks(masks(e, b, n)), history=hist)
    seg.load_category_weights(out)                                      # the returned blob loads
    assert seg.category_info() == (categories, 1, W, H) and seg.categorize(x[val]).shape == (48,)
    drawn = {}
    out2 = train_loop.train_category(seg, blob, x, y, val, epochs=1, batch_size=batch, lr=lr, seed=seed, history=drawn)      # library-drawn masks
    seg.close()
    assert len(out2) == len(blob) and np.isfinite(drawn["losses"][0]) and drawn["steps"] == 3
    # the restatement's run: the same index lists (ResidentLoader's rule), the same masks
    c64 = ref.Chain(state, lr, dtype=torch.float64)
    train_rows = np.arange(96)
    want = []
    for e in range(epochs):
        order = train_rows[np.random.default_rng([seed, e]).permutation(len(train_rows))]
        losses = []
        for b in range(3):
            idx = order[b * batch:(b + 1) * batch]
            losses.append(c64.step(x[idx].astype(np.float32), y[idx], masks(e, b, len(idx)))[0])
        want.append(float(np.mean(losses)))
    assert hist["steps"] == 3 * epochs and len(hist["losses"]) == epochs
    for e in range(epochs):
        print(f"epoch {e}: mean loss {hist['losses'][e]!r} restatement {want[e]!r}")
        assert np.isfinite(hist["losses"][e]) and abs(hist["losses"][e] - want[e]) <= 5e-5 * max(1.0, abs(want[e])), (e, hist["losses"][e], want[e])
    loss64, correct64, _ = ref.evaluate(c64.state(), x[val].astype(np.float32), y[val], dtype=torch.float64)
    print(f"validation: loss {hist['val_loss']!r} restatement {loss64!r}, accuracy {hist['val_accuracy']!r} restatement {correct64 / 48!r}")
    assert abs(hist["val_loss"] - loss64) <= 5e-5 * max(1.0, abs(loss64)) and hist["val_accuracy"] == correct64 / 48
