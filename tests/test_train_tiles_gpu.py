"""The any-size training step (trex_amd/csrc/train_any.hip) at every tile shape of its convolutions, at tiles with an origin past 0, at a second
strip of the conv1 weight gradient, at ragged last shares of the conv2 / conv3 weight gradients and with either axis at 256, against the float64
restatement (oracle/cnn_train_oracle.py, dtype=torch.float64), with injected dropout masks.  The cases are tests/train_tile_cases.py; what each
reaches, and that the float32 restatement stays five times inside the gradient bar of float64 at every one of them, is shown on the CPU by
test_train_tile_cases.py -- so a miss here is the device's.

The bars are test_train_sizes_gpu.py's, taken against float64: loss 5e-5 max(1, |loss64|), `correct` equal, gradients GRAD_RTOL max|g64| per tensor
with every element compared (the three convolution biases feed a BatchNorm: true gradient 0, held to 1e-4 max(1, max|g64 of the weight|)), running
statistics 1e-4 max(1, max|ref|).  Which tensor fails says which kernel: conv1.weight the strips of k_tany_wgrad1, conv2 / conv3.weight the shares of
k_tany_wgrad, everything below a layer that layer's data-gradient tiles, the loss alone the forward tiles.

  1. every case: one step against float64; the device's error per tensor is printed as a multiple of the float32 restatement's own
  2. determinism where the shares are ragged (14 x 100, 100 x 60)
  3. the step's state at 100 x 14: the Adam moments against the device's own gradient, the step count
  4. export and inference at sizes of several tiles (100 x 60, 80 x 72): blob round trip, trexhip_load_weights, prediction in chunks
  5. a second step at a smaller batch on the same trainer (14 x 100, n = 5 then 2): the first step's ragged share leaves nothing behind

The device's error as a multiple of the float32 restatement's error against float64, worst tensor per case (no bar is set on it; MI355X):
   14 x 100   2.29 (conv1.weight)      100 x 14   4.05 (bn3.bias)      100 x 60   2.14 (bn2.bias)
   80 x 72    2.91 (bn1.bias)          8 x 256    2.56 (bn1.bias)      256 x 8    2.66 (bn1.weight)
The worst gradient error itself is bn1.bias's in every case: 1.4e-5 max|g64| at 80 x 72, 1.3e-5 at 100 x 60, at most 4.5e-6 at the other four,
against the bar of 2e-4; the losses are within 2.1e-6, the moments within 1.2e-7 relative, both predictions within 9e-7."""
import numpy as np
import pytest
import torch

from trex_amd import weights
from oracle import cnn_train_oracle as tro, cnn_oracle
from train_tile_cases import CASES, CONV_BIAS, GRAD_RTOL, LR, case_id, find, initial_state, inputs, restatements
from test_train_sizes_gpu import check_step, make_seg, new_trainer, predict, read_all, step

pytestmark = pytest.mark.gpu
NAMES = [nm for nm, _ in weights.TENSORS]


def one_step(seg, shape):
    """a fresh trainer's first step on the case's inputs -> (loss, correct, gradients, parameters, the trainer)"""
    W, H, ch, n, classes = shape
    tr = new_trainer(seg, initial_state(shape), W, H, ch, n, classes)
    assert (tr.width, tr.height, tr.channels, tr.classes) == (W, H, ch, classes)
    loss, correct = step(tr, *inputs(*shape, 0))
    return loss, correct, read_all(tr, classes, ch, W, H, 1), read_all(tr, classes, ch, W, H, 0), tr


def hold_gradients(tag, g, ref, own=None):
    """every element of every gradient tensor within the bar of `ref`; with `own` (the float32 restatement's gradients, ref then float64) the
    device's error is printed as a multiple of own's.  -> the worst such multiple and its tensor"""
    failed, worst = [], (0.0, None)
    for k in tro.TRAINABLE:
        r = np.asarray(ref[k], np.float64)
        assert g[k].shape == r.shape and np.all(np.isfinite(g[k])), k
        if k in CONV_BIAS:
            err, tol = float(np.abs(g[k]).max()), 1e-4 * max(float(np.abs(ref[k.replace("bias", "weight")]).max()), 1.0)
            e32 = float(np.abs(own[k]).max()) if own else None
        else:
            err, tol = float(np.abs(g[k] - r).max()), GRAD_RTOL * float(np.abs(r).max())
            e32 = float(np.abs(own[k] - r).max()) if own else None
        line = f"{tag} grad {k}: err {err:.3g} tol {tol:.3g}"
        if own:
            mult = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
            line += f" = {mult:.3g} x the float32 restatement's {e32:.3g}"
            if k not in CONV_BIAS and mult > worst[0]:
                worst = (mult, k)
        print(line)
        if not err <= tol:
            failed.append((k, err, tol))
    assert not failed, (tag, failed)
    return worst


def hold_statistics(tag, p, ref):
    for k in tro.BUFFERS:
        err = float(np.abs(p[k] - ref[k]).max())
        print(f"{tag} {k}: err {err:.3g}")
        assert err <= 1e-4 * max(1.0, float(np.abs(ref[k]).max())), (tag, k, err)


# ---- 1. one step of every case against float64 ----
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_step_against_float64(case):
    shape = case[0]
    both = restatements(shape)
    _, _, g32, _ = both[torch.float32]
    loss64, correct64, g64, stats64 = both[torch.float64]
    seg = make_seg()
    loss, correct, g, p, tr = one_step(seg, shape)
    assert tr.steps == 1
    tr.close()
    seg.close()
    tag = case_id(case)
    check_step(tag, loss, correct, loss64, correct64)
    mult, where = hold_gradients(tag, g, g64, own=g32)
    print(f"{tag}: worst multiple of the float32 restatement's error {mult:.3g} ({where})")
    hold_statistics(tag, p, stats64)


# ---- 2. determinism where the shares are ragged ----
@pytest.mark.parametrize("W,H", [(14, 100), (100, 60)])
def test_a_second_trainer_gives_the_same_bits_where_the_last_share_is_ragged(W, H):
    shape = find(W, H)
    seg = make_seg()
    runs = []
    for _ in range(2):
        loss, correct, g, p, tr = one_step(seg, shape)
        tr.close()
        runs.append((loss, correct, g, p))
    seg.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    for k in NAMES:
        assert runs[0][2][k].tobytes() == runs[1][2][k].tobytes(), ("gradient", k)
        assert runs[0][3][k].tobytes() == runs[1][3][k].tobytes(), ("parameter", k)


# ---- 3. the step's state ----
def test_the_adam_moments_after_the_first_step_are_the_devices_own_gradient_at_100x14():
    """The moments start at 0, so after one step m = (1 - beta1) g and v = (1 - beta2) g g of the gradient the device itself reports, to 1e-6
    relative (about 8 fp32 ulp: 1 - beta formed in either precision, one fused multiply-add), exactly 0 where g is 0.  The betas are the
    trainer's: trexhip_train_params holds them as floats, so beta2 is float32(0.999) = 0.99900001287..., and 1 - beta2 is 1.3e-5 away from 0.001"""
    shape = find(100, 14)
    W, H, ch, n, classes = shape
    beta1, beta2 = float(np.float32(0.9)), float(np.float32(0.999))
    seg = make_seg()
    loss, correct, g, p, tr = one_step(seg, shape)
    m, v = (read_all(tr, classes, ch, W, H, kind) for kind in (2, 3))
    assert tr.steps == 1
    tr.close()
    seg.close()
    assert np.isfinite(loss)
    for k in tro.TRAINABLE:
        g64 = g[k].astype(np.float64)
        assert np.any(g64 != 0), k
        for what, got, want in (("m", m[k], (1.0 - beta1) * g64), ("v", v[k], (1.0 - beta2) * g64 * g64)):
            zero = g64 == 0
            assert np.all(got[zero] == 0), (what, k)
            # (below fp32's normal range, 1.18e-38, a value is subnormal or flushed and has no relative precision: held absolutely there)
            tiny = np.abs(want) < 2e-38
            rel = np.abs(got[~tiny] - want[~tiny]) / np.abs(want[~tiny])
            print(f"100x14 {what} {k}: max relative error {float(rel.max()) if rel.size else 0.0:.3g}, {int(tiny.sum()) - int(zero.sum())} tiny")
            assert np.all(rel <= 1e-6), (what, k, float(rel.max()))
            assert np.all(np.abs(got[tiny] - want[tiny]) <= 2e-38), (what, k)
    for k in tro.BUFFERS:                                            # running statistics are buffers, not parameters: no moments
        assert not m[k].any() and not v[k].any(), k


# ---- 4. export and inference at sizes of several tiles ----
@pytest.mark.parametrize("W,H", [(100, 60), (80, 72)])
def test_export_and_inference_at_a_size_of_several_tiles(W, H):
    shape = find(W, H)
    _, _, ch, n, classes = shape
    seg = make_seg()
    loss, correct, g, p, tr = one_step(seg, shape)
    blob = tr.export()
    hdr = np.frombuffer(blob[:32], np.int32)
    assert (int(hdr[3]), int(hdr[4])) == (W, H)
    st, c2, ch2 = weights.unpack_blob(blob)
    assert c2 == classes and ch2 == ch
    for k in NAMES:
        assert st[k].tobytes() == p[k].tobytes(), k                  # the blob is the trainer's parameters, bit for bit
    crops = weights.synthetic_crops(16, 9, ch, W, H)
    want, _ = cnn_oracle.predict(st, crops, threads=16)
    # the trainer's own prediction: max_batch = n < 16 crops, so the call walks ceil(16 / n) chunks; a row does not depend on its chunk
    before = [read_all(tr, classes, ch, W, H, kind) for kind in (0, 2, 3)]
    rows16 = predict(tr, crops, classes)
    assert np.abs(rows16 - want).max() <= 1e-4
    shifted = predict(tr, crops[1:], classes)                        # every crop one place on: another chunk, or another row of its chunk
    assert shifted.tobytes() == rows16[1:].tobytes()
    singles = np.concatenate([predict(tr, crops[k:k + 1], classes) for k in (0, n - 1, n, 15)])
    assert singles.tobytes() == rows16[[0, n - 1, n, 15]].tobytes()
    after = [read_all(tr, classes, ch, W, H, kind) for kind in (0, 2, 3)]
    for b, a in zip(before, after):
        for k in b:
            assert np.array_equal(b[k], a[k]), k
    assert tr.steps == 1
    tr.close()
    # ... and what trexhip_load_weights takes
    seg.load_weights(blob)
    probs = seg.probabilities(crops)
    print(f"{W}x{H}: max |dp| trainer {float(np.abs(rows16 - want).max()):.3g}, loaded {float(np.abs(probs - want).max()):.3g}")
    assert np.abs(probs - want).max() <= 1e-4
    seg.close()


# ---- 5. a smaller batch behind a ragged one ----
def test_a_second_step_at_a_smaller_batch_at_14x100():
    """n = 5 (250 rows of conv2's plane in 84 shares of 3, the last one ragged; 125 of conv3's in 42 of 3) and then n = 2 on the same trainer (100 rows
    in 50 shares of 2, 50 in 25 of 2: no clamp, fewer shares than the partials of the step before hold).  Loss, `correct` and the final parameters
    against the float32 restatement's two chained steps with test_three_steps_equal_three_chained_oracle_steps's bars (a float64 chain parts from
    the device's weights by Adam's +-lr).  The second step's gradients and statistics have a reference that no such drift touches: the float64
    restatement of that one step from the parameters and statistics the device itself holds after the first"""
    shape = find(14, 100)
    W, H, ch, n, classes = shape
    assert n == 5
    state = initial_state(shape)
    adam = tro.new_adam_state(state)
    batches = [inputs(W, H, ch, 5, classes, 0), inputs(W, H, ch, 2, classes, 1)]
    ref, cur = [], state
    for x, y, masks in batches:
        cur, loss, correct, grads = tro.train_step(cur, adam, x, y, masks, LR, threads=16)
        ref.append((cur, loss, correct, grads))
    seg = make_seg()
    tr = new_trainer(seg, state, W, H, ch, n, classes)
    for s, (x, y, masks) in enumerate(batches):
        held = read_all(tr, classes, ch, W, H, 0)
        loss, correct = step(tr, x, y, masks)
        g, p = read_all(tr, classes, ch, W, H, 1), read_all(tr, classes, ch, W, H, 0)
        tag = f"14x100 step {s} (n = {len(y)})"
        check_step(tag, loss, correct, ref[s][1], ref[s][2])
        loss64, correct64, g64, stats64, _ = tro.forward_backward(held, x, y, masks, threads=16, dtype=torch.float64)
        check_step(tag + " from the device's own parameters", loss, correct, loss64, correct64)
        hold_gradients(tag, g, g64)
        hold_statistics(tag, p, stats64)
    assert tr.steps == 2
    final = read_all(tr, classes, ch, W, H, 0)
    tr.close()
    seg.close()
    steps = len(batches)
    for k in tro.TRAINABLE:
        r = ref[-1][0][k]
        err = np.abs(final[k] - r)
        # Adam's update is lr m / (sqrt(v) + eps): +-lr per step whatever the gradient's size (test_train_sizes_gpu.py)
        frac = float(np.mean(err <= 0.05 * LR + 1e-6 * np.abs(r)))
        print(f"14x100 final {k}: max err {float(err.max()):.3g} within the narrow bar {frac:.4f}")
        assert err.max() <= 2.0 * steps * LR + 1e-6 * np.abs(r).max(), (k, float(err.max()))
        if k not in CONV_BIAS:
            assert frac >= 0.99, (k, frac)
