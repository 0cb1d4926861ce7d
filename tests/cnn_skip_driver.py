"""The driver the GPU tests of the role-split chain's skipping share (test_cnn_skip_gpu.py, test_cnn_skip3_gpu.py, test_cnn_skipx_gpu.py,
test_cnn_v3_direct_gpu.py): one context per TREXHIP_CONV_GEOM value, the same crops through identify_device, every counter read back.  Each
file picks the counters it asserts on."""
import collections
import numpy as np
import pytest
import torch
from trex_amd import capi, weights

# the counters behind one call: skip_stats() (passes, listed, bytes filled), skipx_stats() (crops windowed, windowed passes, full-width passes),
# skip3_stats() (pairs, listed, passes, bytes filled)
Stats = collections.namedtuple("Stats", "skip skipx skip3")


@pytest.fixture(scope="module")
def state():
    return weights.synthetic_state(100, 31)


def forward(monkeypatch, st, geom, crops, classes=100, calls=1, then=None):
    """-> (probabilities, logits) of every call, guard_stats, Stats of every call; the same device buffers in every call.  `then`: crops
    written into the same device buffer in front of one more call"""
    monkeypatch.setenv("TREXHIP_CONV_GEOM", str(geom))
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(st, classes))
    seg.set_identity_precision(capi.CNN_FP16X3)
    n = len(crops)
    d = torch.from_numpy(np.ascontiguousarray(crops.reshape(n, -1))).cuda()
    probs = torch.empty((n, classes), dtype=torch.float32, device="cuda")
    logits = torch.empty_like(probs)
    outs, stats = [], []
    for call in range(calls + (then is not None)):
        if call == calls:
            d.copy_(torch.from_numpy(np.ascontiguousarray(then.reshape(n, -1))).cuda())
        probs.fill_(-1.0); logits.fill_(-1.0)
        seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
        seg.synchronize()
        outs.append((probs.cpu().numpy().copy(), logits.cpu().numpy().copy()))
        stats.append(Stats(seg.skip_stats(), seg.skipx_stats(), seg.skip3_stats()))
    guard = seg.guard_stats()
    seg.close()
    return outs, guard, stats


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def blob(crops, i, rows, cols, rng):
    crops[i, rows, cols, 0] = rng.integers(40, 200, crops[i, rows, cols, 0].shape)
