"""CPU restatement of one training step, of an evaluation batch and of a prediction of the identity networks v100 and v110 (TEST INFRASTRUCTURE ONLY).

Follows visual_identification_network_torch.py:262-382 in the mode train() puts the model in (visual_recognition_torch.py:1137-1158: forward,
CrossEntropyLoss, backward, Adam; :1171-1190 model.eval() for validation), behind PermuteAxesWrapper (NHWC -> NCHW, Normalize is a pass-through):

  v100   [conv5x5 'same' -> ReLU -> MaxPool2d(2) -> Dropout2d(0.25)] x3 -> flatten (NCHW) -> fc1 -> ReLU -> Dropout(0.5) -> fc2
  v110   [conv5x5 'same' -> MaxPool2d(2) -> BatchNorm2d -> ReLU -> Dropout2d(0.25)] x3 -> flatten -> fc1 -> BatchNorm1d -> ReLU -> Dropout(0.25) -> fc2

The dropout masks are inputs (keep = 1), as in oracle/cnn_train_oracle.py: torch multiplies by bernoulli(1 - p) / (1 - p).  Plain torch functional ops
and autograd in `dtype` (float32: the reference's arithmetic; float64: the reference point the device is held to).  Adam is
oracle.cnn_train_oracle.adam_update.  Pinned against tests/golden/cnn_train_arch.npz, which holds what the reference's own modules produced
(generator: tests/golden/make_train_arch_fixture.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

from trex_amd import weights
from oracle import cnn_train_oracle as tro

EPS_BN = 1e-5
BN_MOMENTUM = 0.1
P_DROP = {"v100": (0.25, 0.25, 0.25, 0.5), "v110": (0.25, 0.25, 0.25, 0.25)}
MASK_PLANES = (("d1", 16), ("d2", 64), ("d3", 100), ("d4", 100))      # the injected masks of one sample: 280 bytes


def names(arch, classes=2, ch=1, W=8, H=8):
    return [n for n, _ in weights.shapes(classes, ch, W, H, arch)]


def buffers(arch):
    return [n for n in names(arch) if "running" in n]


def trainable(arch):
    return [n for n in names(arch) if "running" not in n]


def zero_gradient(arch):
    """tensors whose true gradient is 0 (a bias in front of a BatchNorm) -> the weight whose gradient scales their bar"""
    return {} if arch == "v100" else {"conv1.bias": "conv1.weight", "conv2.bias": "conv2.weight", "conv3.bias": "conv3.weight", "fc1.bias": "fc1.weight"}


def pack_masks(m):
    return np.concatenate([np.ascontiguousarray(m[k], np.uint8).reshape(-1) for k, _ in MASK_PLANES])


def draw_masks(arch, n, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.random((n, c)) >= p for (k, c), p in zip(MASK_PLANES, P_DROP[arch])}


def _net(arch, t, x, masks, train, dtype):
    """x NCHW -> logits; train: batch statistics (t's running statistics are updated in place) + masks; else running statistics, nothing dropped"""
    bn = arch == "v110"
    for i in (1, 2, 3):
        x = F.conv2d(x, t[f"conv{i}.weight"], t[f"conv{i}.bias"], padding=2)
        if bn:
            x = F.max_pool2d(x, 2)
            x = F.batch_norm(x.contiguous(), t[f"bn{i}.running_mean"], t[f"bn{i}.running_var"], t[f"bn{i}.weight"], t[f"bn{i}.bias"], training=train,
                             momentum=BN_MOMENTUM, eps=EPS_BN)
            x = F.relu(x)
        else:
            x = F.max_pool2d(F.relu(x), 2)
        if train:
            noise = torch.from_numpy(np.asarray(masks[f"d{i}"]).astype(np.float64)).div(1.0 - P_DROP[arch][i - 1]).to(dtype)
            x = x * noise[:, :, None, None]
    x = F.linear(x.reshape(x.shape[0], -1), t["fc1.weight"], t["fc1.bias"])
    if bn:
        x = F.batch_norm(x, t["bn4.running_mean"], t["bn4.running_var"], t["bn4.weight"], t["bn4.bias"], training=train, momentum=BN_MOMENTUM, eps=EPS_BN)
    x = F.relu(x)
    if train:
        x = x * torch.from_numpy(np.asarray(masks["d4"]).astype(np.float64)).div(1.0 - P_DROP[arch][3]).to(dtype)
    return F.linear(x, t["fc2.weight"], t["fc2.bias"])


def _tensors(arch, state, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(state[k], np.float32)).clone().to(dtype) for k in trainable(arch) + buffers(arch)}


def _input(x_nhwc, dtype):
    return torch.from_numpy(np.ascontiguousarray(x_nhwc, np.float32)).to(dtype).permute(0, 3, 1, 2)


def forward_backward(arch, state, x_nhwc, targets, masks, dtype=torch.float32, threads=None):
    """-> loss, correct, grads {name: ndarray}, running statistics after the step {name: ndarray}"""
    if threads:
        torch.set_num_threads(threads)
    arch = weights.arch_name(arch)
    if arch == "v110" and len(targets) < 2:
        raise ValueError("Expected more than 1 value per channel when training")
    t = _tensors(arch, state, dtype)
    for k in trainable(arch):
        t[k].requires_grad_(True)
    y = torch.from_numpy(np.asarray(targets).astype(np.int64))
    logits = _net(arch, t, _input(x_nhwc, dtype), masks, True, dtype)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = {k: t[k].grad.numpy().copy() for k in trainable(arch)}
    stats = {k: t[k].detach().numpy().copy() for k in buffers(arch)}
    return float(loss.detach()), int((logits.argmax(1) == y).sum()), grads, stats


def evaluate(arch, state, x_nhwc, targets, dtype=torch.float32):
    """model.eval(): -> mean cross entropy, correct count, softmax rows"""
    arch = weights.arch_name(arch)
    with torch.no_grad():
        logits = _net(arch, _tensors(arch, state, dtype), _input(x_nhwc, dtype), None, False, dtype)
        y = torch.from_numpy(np.asarray(targets).astype(np.int64))
        return float(F.cross_entropy(logits, y)), int((logits.argmax(1) == y).sum()), torch.softmax(logits, 1).numpy()


def predict(arch, state, crops_u8, dtype=torch.float32):
    """uint8 NHWC crops -> softmax rows in eval mode"""
    n = len(crops_u8)
    return evaluate(arch, state, np.asarray(crops_u8, np.float32), np.zeros(n, np.int64), dtype)[2]


def new_adam_state(arch, state):
    return {"step": 0, "m": {k: np.zeros_like(state[k]) for k in tro.TRAINABLE if k in state}, "v": {k: np.zeros_like(state[k]) for k in tro.TRAINABLE if k in state}}


def adam_update(arch, state, adam, grads, lr):
    """oracle.cnn_train_oracle.adam_update on the version's trainable tensors (that function walks V118_3's names: the ones this version lacks
    ride along as empty arrays)"""
    missing = [k for k in tro.TRAINABLE if k not in state]
    empty = np.zeros(0, np.float32)
    st = dict(state)
    g = {k: np.ascontiguousarray(v, np.float32) for k, v in grads.items()}
    for k in missing:
        st[k] = empty; g[k] = empty; adam["m"][k] = empty.copy(); adam["v"][k] = empty.copy()
    out = tro.adam_update(st, adam, g, lr)
    for k in missing:
        del out[k], adam["m"][k], adam["v"][k]
    return out


def train_step(arch, state, adam, x_nhwc, targets, masks, lr, dtype=torch.float32):
    """one optimizer step -> (new state with the running statistics, loss, correct, grads)"""
    loss, correct, grads, stats = forward_backward(arch, state, x_nhwc, targets, masks, dtype)
    new = adam_update(arch, state, adam, grads, lr)
    new.update({k: v.astype(np.float32) for k, v in stats.items()})
    return new, loss, correct, grads
