"""Restatement of TRex's categorisation in torch functional ops and plain Python, the reference of the category tests.

  forward      the category network in eval mode (trex_learn_category.py:18-44 PyTorchModel, :289 / :435 the normalisation, :441 the label) in
               float32 or float64.  The zero padding of every convolution is applied to the NORMALISED image.
  vote         the reduction of a tracklet's labels: DataStore::label_averaged (CategorizeDatastore.cpp:555-585) and the shares of a sample
               (CategorizeInterface.cpp:212-247), line by line
  sample_rows  which rows of a tracklet are predicted at all: DataStore::temporary (CategorizeDatastore.cpp:1103-1152)
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5      # nn.BatchNorm2d's default


def normalise(crops_u8, dtype=torch.float32):
    """uint8 NHWC -> NCHW `dtype`: x / 127.5 - 1, a true division and a subtraction, each rounded in `dtype`"""
    x = torch.from_numpy(np.ascontiguousarray(crops_u8)).to(dtype) / 127.5 - 1
    return x.permute(0, 3, 1, 2).contiguous()


def _t(state, name, dtype):
    return torch.from_numpy(np.ascontiguousarray(state[name])).to(dtype)


def trunk(state, x, dtype, upto=3, fold_offset=False):
    """the convolution blocks 1..upto on a normalised (or, with fold_offset, raw-scaled) NCHW image"""
    for i in range(1, upto + 1):
        x = F.conv2d(x, _t(state, f"conv{i}.weight", dtype), _t(state, f"conv{i}.bias", dtype), padding=1)
        x = F.batch_norm(x, _t(state, f"batch_norm{i}.running_mean", dtype), _t(state, f"batch_norm{i}.running_var", dtype),
                         _t(state, f"batch_norm{i}.weight", dtype), _t(state, f"batch_norm{i}.bias", dtype), training=False, eps=EPS)
        x = F.max_pool2d(F.relu(x), kernel_size=2, stride=2)      # floors; Dropout(0.25) is the identity in eval mode
    return x


def head(state, x, dtype):
    x = x.reshape(x.size(0), -1)                                  # the NCHW flatten
    x = F.relu(F.linear(x, _t(state, "fc1.weight", dtype), _t(state, "fc1.bias", dtype)))
    return F.linear(x, _t(state, "fc2.weight", dtype), _t(state, "fc2.bias", dtype))


def forward(state, crops_u8, dtype=torch.float32):
    """-> (probs, logits, labels) as numpy arrays of `dtype` / int32; label = the first maximum of the softmax row"""
    with torch.no_grad():
        logits = head(state, trunk(state, normalise(crops_u8, dtype), dtype), dtype)
        probs = torch.softmax(logits, dim=1)
        labels = probs.argmax(dim=1)
    return probs.numpy(), logits.numpy(), labels.numpy().astype(np.int32)


def forward_offset_in_bias(state, crops_u8, dtype=torch.float32):
    """The WRONG network that folds the normalisation's offset into conv1's bias: conv1 on x / 127.5 with bias - sum(w).  Equal to forward() where no
    tap is padded, different on the border -- the tests show that the difference is visible in the logits."""
    with torch.no_grad():
        x = (torch.from_numpy(np.ascontiguousarray(crops_u8)).to(dtype) / 127.5).permute(0, 3, 1, 2).contiguous()
        st = dict(state)
        w = np.asarray(state["conv1.weight"], np.float64)
        st["conv1.bias"] = (np.asarray(state["conv1.bias"], np.float64) - w.sum(axis=(1, 2, 3))).astype(np.float32 if dtype == torch.float32 else np.float64)
        logits = head(st, trunk(st, x, dtype), dtype)
    return logits.numpy()


def vote(labels, tracklet, n_tracklets, categories):
    """-> counts uint32 [T][C], rows uint32 [T], label int32 [T], share float32 [T][C], skipped"""
    T, C = int(n_tracklets), int(categories)
    counts = np.zeros((T, C), np.uint32)
    rows = np.zeros(T, np.uint32)
    skipped = 0
    for l, t in zip(np.asarray(labels).tolist(), np.asarray(tracklet).tolist()):
        if not 0 <= t < T:
            raise ValueError(f"tracklet id {t} outside 0..{T - 1}")
        rows[t] += 1                      # S = task.result.size(): every row handed in
        if l < 0:                         # no label: `if(l)` / `raw_label < 0 -> continue`
            continue
        if l >= C:                        # "Label index > counts.size()": warned about, skipped
            skipped += 1
            continue
        counts[t, l] += 1
    label = np.full(T, -1, np.int32)
    share = np.zeros((T, C), np.float32)
    for t in range(T):
        i = int(np.argmax(counts[t]))     # std::max_element: the first maximum
        if counts[t, i] != 0:             # `if(*mit == 0) return nullptr`
            label[t] = i
        if rows[t]:
            share[t] = counts[t].astype(np.float32) / np.float32(rows[t])
    return counts, rows, label, share, skipped


def sample_rows(size, first_frame, sample_rate, min_samples):
    """-> (rows int32, valid): the indices into the tracklet's basic_index that are predicted"""
    step = 1 if size < min_samples else max(1, size // sample_rate)
    start_offset = 5 - first_frame % 5 if size >= 15 else 0
    rows = []
    i = 0
    while i + start_offset < size:
        rows.append(i + start_offset)
        i += step
    return np.asarray(rows, np.int32), len(rows) >= min_samples
