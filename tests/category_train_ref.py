"""CPU restatement of one training step, of an evaluation batch and of a prediction of the category network (TEST INFRASTRUCTURE ONLY).

Follows trex_learn_category.py:18-44 (PyTorchModel) in the mode perform_training puts it in (:314-332 on a non-CUDA device: forward, CrossEntropyLoss,
backward, Adam with torch's defaults; :338 model.eval() for the evaluation):

  x = images / 127.5 - 1 (:289: a true division, then the subtraction), zero padding AFTER the normalisation
  [conv3x3 padding 1 -> BatchNorm2d -> ReLU -> MaxPool2d(2) -> Dropout(0.25)] x3 (16, 64, 100) -> flatten (NCHW) -> fc1 -> ReLU -> Dropout(0.25) -> fc2

The dropout is ELEMENT-wise (nn.Dropout, not Dropout2d).  Its masks are inputs (1 = keep) in the ABI's layout: d1..d3 NHWC [n][h_i][w_i][C_i] on the
pooled planes, d4 [n][100]; torch multiplies by bernoulli(1 - p) / (1 - p).  Plain torch functional ops and autograd in `dtype` (float32: the
reference's arithmetic; float64: the reference point the device is held to).  Pinned against tests/golden/category_train.npz, which holds what the
reference's own module produced (generator: tests/golden/make_category_train_fixture.py).

`mutant` restates two WRONG first layers, for the tests that show a check can see them: "pad_minus_one" pads the raw image with 0 before the
normalisation (the border then holds -1), "offset_in_bias" runs conv1 on x / 127.5 and folds -sum(w) into its bias.
"""
import numpy as np
import torch
import torch.nn.functional as F

from trex_amd import weights

EPS_BN = 1e-5
BN_MOMENTUM = 0.1
P_DROP = 0.25
CONVS = weights.CATEGORY_CONVS


def names(categories=2, ch=1, W=8, H=8):
    return [n for n, _ in weights.category_shapes(categories, ch, W, H)]


def buffers():
    return [n for n in names() if "running" in n]


def trainable():
    return [n for n in names() if "running" not in n]


def pooled_planes(W, H):
    """(h_i, w_i) of the three pooled planes, by successive floors"""
    out, h, w = [], H, W
    for _ in range(3):
        h, w = h // 2, w // 2
        out.append((h, w))
    return out


def mask_shapes(n, W, H):
    return [(f"d{i + 1}", (n, h, w, c)) for i, ((h, w), c) in enumerate(zip(pooled_planes(W, H), CONVS))] + [("d4", (n, 100))]


def mask_bytes(n, W, H):
    return sum(int(np.prod(s)) for _, s in mask_shapes(n, W, H))


def draw_masks(n, W, H, seed, p=P_DROP):
    rng = np.random.default_rng(seed)
    return {k: rng.random(s) >= p for k, s in mask_shapes(n, W, H)}


def ones_masks(n, W, H):
    return {k: np.ones(s, bool) for k, s in mask_shapes(n, W, H)}


def pack_masks(m):
    return np.concatenate([np.ascontiguousarray(m[k], np.uint8).reshape(-1) for k in ("d1", "d2", "d3", "d4")])


def _noise(mask, dtype, nhwc):
    t = torch.from_numpy(np.asarray(mask).astype(np.float64)).div(1.0 - P_DROP).to(dtype)
    return t.permute(0, 3, 1, 2) if nhwc else t


def _first_layer(t, x_nhwc, dtype, mutant):
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc, np.float32)).to(dtype).permute(0, 3, 1, 2)
    w, b = t["conv1.weight"], t["conv1.bias"]
    if mutant is None:
        return F.conv2d(x / 127.5 - 1, w, b, padding=1)
    if mutant == "pad_minus_one":
        return F.conv2d(F.pad(x, (1, 1, 1, 1)) / 127.5 - 1, w, b)
    if mutant == "offset_in_bias":
        return F.conv2d(x / 127.5, w, b - w.sum(dim=(1, 2, 3)), padding=1)
    raise ValueError(mutant)


def _net(t, x_nhwc, masks, train, dtype, mutant=None):
    """x NHWC in [0, 255] -> logits; train: batch statistics (t's running statistics are updated in place) + masks; else running statistics"""
    x = None
    for i in (1, 2, 3):
        x = _first_layer(t, x_nhwc, dtype, mutant) if i == 1 else F.conv2d(x, t[f"conv{i}.weight"], t[f"conv{i}.bias"], padding=1)
        x = F.batch_norm(x, t[f"batch_norm{i}.running_mean"], t[f"batch_norm{i}.running_var"], t[f"batch_norm{i}.weight"], t[f"batch_norm{i}.bias"],
                         training=train, momentum=BN_MOMENTUM, eps=EPS_BN)
        x = F.max_pool2d(F.relu(x), kernel_size=2, stride=2)
        if train:
            x = x * _noise(masks[f"d{i}"], dtype, True)
    x = F.relu(F.linear(x.reshape(x.shape[0], -1), t["fc1.weight"], t["fc1.bias"]))
    if train:
        x = x * _noise(masks["d4"], dtype, False)
    return F.linear(x, t["fc2.weight"], t["fc2.bias"])


def _tensors(state, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(state[k], np.float32)).clone().to(dtype) for k in names()}


def forward_backward(state, x_nhwc, targets, masks, dtype=torch.float32, threads=None, mutant=None):
    """-> loss, correct, grads {name: ndarray}, running statistics after the step {name: ndarray}"""
    if threads:
        torch.set_num_threads(threads)
    t = _tensors(state, dtype)
    for k in trainable():
        t[k].requires_grad_(True)
    y = torch.from_numpy(np.asarray(targets).astype(np.int64))
    logits = _net(t, x_nhwc, masks, True, dtype, mutant)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = {k: t[k].grad.numpy().copy() for k in trainable()}
    stats = {k: t[k].detach().numpy().copy() for k in buffers()}
    return float(loss.detach()), int((logits.argmax(1) == y).sum()), grads, stats


def evaluate(state, x_nhwc, targets, dtype=torch.float32):
    """model.eval(): -> mean cross entropy, correct count, softmax rows"""
    with torch.no_grad():
        logits = _net(_tensors(state, dtype), x_nhwc, None, False, dtype)
        y = torch.from_numpy(np.asarray(targets).astype(np.int64))
        return float(F.cross_entropy(logits, y)), int((logits.argmax(1) == y).sum()), torch.softmax(logits, 1).numpy()


def predict(state, crops_u8, dtype=torch.float32):
    """uint8 NHWC crops -> softmax rows in eval mode"""
    n = len(crops_u8)
    return evaluate(state, np.asarray(crops_u8, np.float32), np.zeros(n, np.int64), dtype)[2]


class Chain:
    """the model and torch.optim.Adam (the reference's optimizer, :295 with its defaults but lr) over several steps, in `dtype`"""

    def __init__(self, state, lr, dtype=torch.float64):
        self.dtype = dtype
        self.t = _tensors(state, dtype)
        for k in trainable():
            self.t[k].requires_grad_(True)
        self.opt = torch.optim.Adam([self.t[k] for k in trainable()], lr=lr)

    def step(self, x_nhwc, targets, masks):
        """-> loss, correct, the gradients of this step"""
        y = torch.from_numpy(np.asarray(targets).astype(np.int64))
        self.opt.zero_grad()
        logits = _net(self.t, x_nhwc, masks, True, self.dtype)
        loss = F.cross_entropy(logits, y)
        loss.backward()
        grads = {k: self.t[k].grad.numpy().copy() for k in trainable()}
        self.opt.step()
        return float(loss.detach()), int((logits.argmax(1) == y).sum()), grads

    def state(self):
        return {k: v.detach().numpy().copy() for k, v in self.t.items()}

    def moments(self):
        """-> (exp_avg, exp_avg_sq) {name: ndarray} of the trainable tensors"""
        m = {k: self.opt.state[self.t[k]]["exp_avg"].numpy().copy() for k in trainable()}
        v = {k: self.opt.state[self.t[k]]["exp_avg_sq"].numpy().copy() for k in trainable()}
        return m, v
