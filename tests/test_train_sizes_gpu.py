"""The training step of the identity network at individual_image_sizes other than 80x80 (trex_amd/csrc/train_any.hip) against the CPU
restatement oracle/cnn_train_oracle.py, with injected dropout masks.  fp32 on both sides.

Shapes (W x H, channels, batch, classes) and what each can catch:
   8 x 8,  1, 16, 5     the smallest: conv3 sees 2 x 2, one fc1 position, one ragged tile everywhere
  21 x 13, 3, 12, 7     odd at levels 1 and 3 on both axes (21 -> 10 -> 5 -> 2, 13 -> 6 -> 3 -> 1), W != H, two fc1 positions, three channels
  13 x 21, 1, 12, 7     the transpose: a swapped W / H anywhere
  40 x 72, 1, 8, 100    several tiles with a ragged last one in conv2 and conv3, 45 fc1 positions, the reference's class count
Inputs: weights.synthetic_train_batch's recipe on weights.synthetic_crops(n, seed + 7, ch, W, H), seed 1000 + 7 W + H (+ 100 per further step);
masks drawn as in test_train_gpu.py.  The bars are that file's: loss 5e-5 max(1, |ref|), `correct` equal, gradients 2e-4 max|g_ref| per tensor
(the three convolution biases feed a BatchNorm: true gradient 0, held to 1e-4 max(1, max|g_ref of the weight|)), running statistics
1e-4 max(1, max|ref|); every element is compared.  The fp32 restatement against its float64 self at these shapes and seeds: worst gradient
difference 3.7e-5 max|g| (40 x 72, conv2.weight), 1.5e-6 at the other three, loss within 1.3e-6: a factor of five inside the bar."""
import ctypes as C
import functools
import numpy as np
import pytest
import torch

from trex_amd import capi, weights
from oracle import cnn_train_oracle as tro, cnn_oracle

pytestmark = pytest.mark.gpu
GRAD_RTOL = 2e-4
CONV_BIAS = ("conv1.bias", "conv2.bias", "conv3.bias")
LR = 1e-3
SHAPES = [(8, 8, 1, 16, 5), (21, 13, 3, 12, 7), (13, 21, 1, 12, 7), (40, 72, 1, 8, 100)]
E_INVALID, E_UNSUPPORTED = -1, -4


def make_seg():
    p = capi.default_params(64, 64)
    p.max_batch = 1
    return capi.Segmenter(p)


def train_batch(n, seed, classes, ch, W, H):
    """weights.synthetic_train_batch at W x H (that helper is 80x80 only)"""
    rng = np.random.default_rng(seed)
    x = weights.synthetic_crops(n, seed + 7, ch, W, H).astype(np.float32)
    x = np.clip(x * rng.uniform(0.85, 1.15, (n, 1, 1, 1)).astype(np.float32) + rng.uniform(0.0, 3.0, x.shape).astype(np.float32) * (x > 0), 0.0, 255.0)
    y = rng.integers(0, classes, n).astype(np.int32)
    return np.ascontiguousarray(x, np.float32), y


def draw_masks(n, seed):
    rng = np.random.default_rng(seed)
    return {"d1": rng.random((n, 16)) >= 0.05, "d2": rng.random((n, 64)) >= 0.05, "d3": rng.random((n, 128)) >= 0.05, "d4": rng.random((n, 100)) >= 0.05}


def pack_masks(m):
    return np.concatenate([np.ascontiguousarray(m[k], np.uint8).reshape(-1) for k in ("d1", "d2", "d3", "d4")])


def inputs(W, H, ch, n, classes, s):
    seed = 1000 + 7 * W + H + 100 * s
    x, y = train_batch(n, seed, classes, ch, W, H)
    return x, y, draw_masks(n, seed)


@functools.lru_cache(maxsize=None)
def reference(W, H, ch, n, classes, steps):
    """the restatement's chained steps, computed once per shape: [(state after, loss, correct, grads)] and the initial state"""
    state = weights.synthetic_state(classes, 1000 + 7 * W + H, channels=ch, width=W, height=H)
    adam = tro.new_adam_state(state)
    out, cur = [], state
    for s in range(steps):
        x, y, masks = inputs(W, H, ch, n, classes, s)
        cur, loss, correct, grads = tro.train_step(cur, adam, x, y, masks, LR, threads=16)
        out.append((cur, loss, correct, grads))
    return state, out


def read_all(tr, classes, ch, W, H, kind):
    return {n: tr.read(i, kind, shp) for i, (n, shp) in enumerate(weights.shapes(classes, ch, W, H))}


def step(tr, x, y, masks):
    dx = torch.from_numpy(x).cuda()
    dy = torch.from_numpy(y.astype(np.int32)).cuda()
    dm = torch.from_numpy(pack_masks(masks)).cuda()
    out = tr.step_device(dx.data_ptr(), dy.data_ptr(), x.shape[0], dm.data_ptr())
    torch.cuda.synchronize()
    return out


def new_trainer(seg, state, W, H, ch, n, classes, **kw):
    return capi.Trainer(seg, weights.pack_blob(state, classes, ch, W, H), max_batch=n, lr=LR, **kw)


def check_step(tag, loss, correct, ref_loss, ref_correct):
    print(f"{tag}: loss {loss!r} ref {ref_loss!r} correct {correct} ref {ref_correct}")
    assert abs(loss - ref_loss) <= 5e-5 * max(1.0, abs(ref_loss)), (tag, loss, ref_loss)
    assert correct == ref_correct, (tag, correct, ref_correct)


@pytest.mark.parametrize("W,H,ch,n,classes", SHAPES)
def test_one_step_equals_the_oracle_is_deterministic_and_exports(W, H, ch, n, classes):
    state, ref = reference(W, H, ch, n, classes, 3 if (W, H) in ((8, 8), (21, 13)) else 1)
    new, loss_ref, correct_ref, grads = ref[0]
    x, y, masks = inputs(W, H, ch, n, classes, 0)
    seg = make_seg()
    runs = []
    for _ in range(2):
        tr = new_trainer(seg, state, W, H, ch, n, classes)
        assert (tr.width, tr.height, tr.channels, tr.classes) == (W, H, ch, classes)
        loss, correct = step(tr, x, y, masks)
        runs.append((loss, correct, read_all(tr, classes, ch, W, H, 1), read_all(tr, classes, ch, W, H, 0), tr.export()))
        tr.close()
    loss, correct, g, p, blob = runs[0]
    check_step(f"{W}x{H}", loss, correct, loss_ref, correct_ref)
    failed = []
    for k in tro.TRAINABLE:
        if k in CONV_BIAS:
            err, tol = float(np.abs(g[k]).max()), 1e-4 * max(float(np.abs(grads[k.replace("bias", "weight")]).max()), 1.0)
        else:
            err, tol = float(np.abs(g[k] - grads[k]).max()), GRAD_RTOL * float(np.abs(grads[k]).max()) + 1e-9
        print(f"{W}x{H} grad {k}: err {err:.3g} tol {tol:.3g}")
        if not err <= tol:
            failed.append((k, err, tol))
    assert not failed, failed
    for k in tro.BUFFERS:
        err = float(np.abs(p[k] - new[k]).max())
        print(f"{W}x{H} {k}: err {err:.3g}")
        assert err <= 1e-4 * max(1.0, float(np.abs(new[k]).max())), (k, err)
    # every reduction has a fixed order: a second trainer on the same inputs gives the same bits
    assert runs[1][0] == loss and runs[1][1] == correct
    names = [nm for nm, _ in weights.TENSORS]
    for k in names:
        assert np.array_equal(runs[1][2][k], g[k]) and np.array_equal(runs[1][3][k], p[k]), k
    # the exported blob is the trainer's parameters, and what trexhip_load_weights takes
    hdr = np.frombuffer(blob[:32], np.int32)
    assert (int(hdr[3]), int(hdr[4])) == (W, H)
    st2, c2, ch2 = weights.unpack_blob(blob)
    assert c2 == classes and ch2 == ch
    for k in names:
        assert np.array_equal(st2[k], p[k]), k
    seg.load_weights(blob)
    crops = weights.synthetic_crops(16, 9, ch, W, H)
    probs = seg.probabilities(crops)
    ref_probs, _ = cnn_oracle.predict(st2, crops, threads=16)
    assert np.abs(probs - ref_probs).max() <= 1e-4
    seg.close()


@pytest.mark.parametrize("W,H,ch,n,classes", SHAPES[:2])
def test_three_steps_equal_three_chained_oracle_steps(W, H, ch, n, classes):
    steps = 3
    state, ref = reference(W, H, ch, n, classes, steps)
    seg = make_seg()
    tr = new_trainer(seg, state, W, H, ch, n, classes)
    for s in range(steps):
        x, y, masks = inputs(W, H, ch, n, classes, s)
        loss, correct = step(tr, x, y, masks)
        check_step(f"{W}x{H} step {s}", loss, correct, ref[s][1], ref[s][2])
    assert tr.steps == steps
    final = read_all(tr, classes, ch, W, H, 0)
    tr.close()
    seg.close()
    for k in tro.TRAINABLE:
        r = ref[-1][0][k]
        err = np.abs(final[k] - r)
        # Adam's update is lr m / (sqrt(v) + eps): +-lr per step whatever the gradient's size, so elements whose gradient is rounding noise
        # move by up to lr per step in an arbitrary direction (test_train_gpu.py: test_training_steps_equal_the_reference_module)
        frac = float(np.mean(err <= 0.05 * LR + 1e-6 * np.abs(r)))
        print(f"{W}x{H} final {k}: max err {float(err.max()):.3g} within the narrow bar {frac:.4f}")
        assert err.max() <= 2.0 * steps * LR + 1e-6 * np.abs(r).max(), (k, float(err.max()))
        if k not in CONV_BIAS:
            assert frac >= 0.99, (k, frac)


def predict(tr, crops, classes):
    d = torch.from_numpy(crops).cuda()
    out = torch.full((len(crops), classes), -1.0, dtype=torch.float32, device="cuda")
    tr.predict_device(d.data_ptr(), len(crops), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_prediction_at_21x13_walks_chunks_and_changes_nothing():
    W, H, ch, n, classes = SHAPES[1]
    state, _ = reference(W, H, ch, n, classes, 3)
    seg = make_seg()
    tr = new_trainer(seg, state, W, H, ch, 4, classes)          # max_batch 4: 5 crops are two chunks, 13 four
    x, y, masks = inputs(W, H, ch, 4, classes, 0)
    step(tr, x, y, masks)                                        # the weights, moments and statistics are the trainer's own
    before = [read_all(tr, classes, ch, W, H, kind) for kind in (0, 2, 3)]
    crops = weights.synthetic_crops(13, 21, ch, W, H)
    rows13 = predict(tr, crops, classes)
    rows5 = predict(tr, crops[:5], classes)
    st, _, _ = weights.unpack_blob(tr.export())
    want, _ = cnn_oracle.predict(st, crops, threads=16)
    print(f"predict 21x13: max |dp| = {float(np.abs(rows13 - want).max()):.3g}")
    assert np.abs(rows13 - want).max() <= 1e-4 and np.abs(rows5 - want[:5]).max() <= 1e-4
    assert rows13[:5].tobytes() == rows5.tobytes()               # a row does not depend on its chunk
    singles = np.concatenate([predict(tr, crops[k:k + 1], classes) for k in range(5)])
    assert singles.tobytes() == rows5.tobytes()
    after = [read_all(tr, classes, ch, W, H, kind) for kind in (0, 2, 3)]
    for b, a in zip(before, after):
        for k in b:
            assert np.array_equal(b[k], a[k]), k
    assert tr.steps == 1
    tr.close()
    seg.close()


def test_both_precisions_run_the_same_exact_chain_at_21x13():
    W, H, ch, n, classes = SHAPES[1]
    state, _ = reference(W, H, ch, n, classes, 3)
    x, y, masks = inputs(W, H, ch, n, classes, 0)
    seg = make_seg()
    runs = []
    for precision in (0, 1):
        tr = new_trainer(seg, state, W, H, ch, n, classes, precision=precision)
        loss, correct = step(tr, x, y, masks)
        runs.append((loss, correct, read_all(tr, classes, ch, W, H, 1), read_all(tr, classes, ch, W, H, 0)))
        tr.close()
    seg.close()
    assert runs[0][:2] == runs[1][:2]
    for k in runs[0][2]:
        assert np.array_equal(runs[0][2][k], runs[1][2][k]) and np.array_equal(runs[0][3][k], runs[1][3][k]), k


@pytest.mark.parametrize("W,H", [(7, 80), (264, 80)])
def test_blob_sizes_outside_the_range_are_refused(W, H):
    classes = 3
    # a well-formed blob of that size (7 x 80 has no fc1 input at all, so the tensors are plain zeros, the variances ones)
    state = {k: (np.ones if k.endswith("running_var") else np.zeros)(shp, np.float32) for k, shp in weights.shapes(classes, 1, W, H)}
    blob = weights.pack_blob(state, classes, 1, W, H)
    seg = make_seg()
    p = capi.TrainParams(max_batch=4, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, bn_momentum=0.1, dropout=0.05, seed=0, precision=0)
    h = C.c_void_p()
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    rc = capi.lib().trexhip_trainer_create(seg.handle, buf, len(blob), C.byref(p), C.byref(h))
    assert rc == E_UNSUPPORTED and h.value is None
    assert b"individual_image_size" in capi.lib().trexhip_last_error()
    seg.close()


def test_a_target_out_of_range_is_refused_at_13x21_with_parameters_untouched():
    W, H, ch, n, classes = SHAPES[2]
    state, _ = reference(W, H, ch, n, classes, 1)
    x, y, masks = inputs(W, H, ch, n, classes, 0)
    seg = make_seg()
    tr = new_trainer(seg, state, W, H, ch, n, classes)
    bad = y.copy()
    bad[3] = classes
    with pytest.raises(capi.TrexHipError):
        step(tr, x, bad, masks)
    assert tr.steps == 0
    now = read_all(tr, classes, ch, W, H, 0)
    for k, v in state.items():
        assert np.array_equal(now[k], v), k
    for kind in (2, 3):
        assert all(not m.any() for m in read_all(tr, classes, ch, W, H, kind).values())
    with pytest.raises(ValueError):
        tr.step(x[:, :, :-1], y)                                 # the host entry point checks against the trainer's size, not 80 x 80
    loss, correct = step(tr, x, y, masks)                        # and the trainer goes on
    assert np.isfinite(loss) and tr.steps == 1
    tr.close()
    seg.close()
