"""trexhip_identify_prepare_device queues, ahead of an identify call, the launches of the role-split chain that read only the crops and the
loaded network (the band / list / fill kernels of trex_amd/csrc/cnn_skip_kernels.h); the identify call it was made for skips them
(trex_amd/csrc/cnn_prepared.h), every other call runs its whole chain.  Either way every probability, logit and counter must be, bit for bit,
that of the call without a prepare in front of it.

1056 crops with the role split forced (TREXHIP_CONV_GEOM bit 29): above 1024, so the listed fc1 and k_head run; 33 blocks of 32 crops for the
pair lists, two workgroups of the pass lists, the last partial.  A batch this small takes the captured-graph path from a context's second call
on, where a prepare call is a no-op by contract: the cases below keep the stage timers on (no chain is captured while they are), and read the
PREPARE stage's launch count to know that the prepare calls did queue their kernels."""
import numpy as np
import pytest
import torch
from trex_amd import capi, weights
from cnn_skip_driver import blob, state  # noqa: F401  (state: the module's fixture)

pytestmark = pytest.mark.gpu

RS = 1 << 29
N, CLASSES = 1056, 100


def make_crops(seed=5):
    """the kinds the skip tests use, in turn: empty, one pixel, a bar of exactly 3 and of 5 conv3 tiles (tile t reads the crop columns
    16 t - 14 .. 16 t + 29), blobs wider than a window of 8 conv1+conv2 tiles, ellipses, noise"""
    rng = np.random.default_rng(seed)
    crops = weights.synthetic_crops(N, 900 + seed).copy()
    for i in range(0, N, 8):
        crops[i] = 0
    for i in range(1, N, 8):
        crops[i] = 0
        crops[i, int(rng.integers(0, 80)), int(rng.integers(0, 80)), 0] = 255
    for i in range(2, N, 8):
        crops[i] = 0
        y0 = int(rng.integers(0, 60))
        blob(crops, i, slice(y0, y0 + int(rng.integers(1, 20))), slice(30, 35), rng)      # tiles 1 .. 3 exactly
    for i in range(3, N, 8):
        crops[i] = 0
        y0 = int(rng.integers(0, 40))
        blob(crops, i, slice(y0, y0 + int(rng.integers(1, 40))), slice(10, 70), rng)      # all five tiles
    for i in range(4, N, 8):
        crops[i] = 0
        y0, x0 = int(rng.integers(0, 50)), int(rng.integers(0, 8))
        blob(crops, i, slice(y0, y0 + 30), slice(x0, x0 + 66 + 3 * (i % 3)), rng)         # 66 .. 72 columns: nine tiles of 8 and more
    for i in range(5, N, 64):
        crops[i, :, :, 0] = rng.integers(1, 256, (80, 80))
    return crops


class Ctx:
    """one context with the timers on, its crops in one device buffer"""

    def __init__(self, monkeypatch, st, geom, crops, timers=True):
        monkeypatch.setenv("TREXHIP_CONV_GEOM", str(geom))
        self.blob = weights.pack_blob(st, CLASSES)
        self.seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
        self.seg.load_weights(self.blob)
        self.seg.set_identity_precision(capi.CNN_FP16X3)
        self.n = len(crops)
        self.d = torch.from_numpy(np.ascontiguousarray(crops.reshape(self.n, -1))).cuda()
        self.probs = torch.empty((self.n, CLASSES), dtype=torch.float32, device="cuda")
        self.logits = torch.empty_like(self.probs)
        if timers:
            self.seg.profile_enable(True)

    def prepare(self, d=None, n=None):
        self.seg.identify_prepare_device((self.d if d is None else d).data_ptr(), self.n if n is None else n)

    def prepared_launches(self):
        return self.seg.profile_read(capi.STAGE_PREPARE)[1]

    def identify(self, n=None):
        """-> (probabilities, logits, every counter) of one call on the context's crops"""
        n = self.n if n is None else n
        seg = self.seg
        self.probs.fill_(-1.0); self.logits.fill_(-1.0)
        seg.identify_device(self.d.data_ptr(), n, self.probs.data_ptr(), self.logits.data_ptr())
        seg.synchronize()
        stats = (seg.skip_stats(), seg.skipx_stats(), seg.skip3_stats(), seg.skip3x_stats(), seg.fc1_stats(), seg.bgrow_stats(), seg.guard_stats())
        return self.probs[:n].cpu().numpy().tobytes(), self.logits[:n].cpu().numpy().tobytes(), stats

    def close(self):
        self.seg.close()


@pytest.fixture(scope="module")
def crops():
    return make_crops()


def test_prepared_equals_unprepared_and_every_mismatch_runs_the_whole_chain(monkeypatch, state, crops):
    c = Ctx(monkeypatch, state, RS, crops)
    want = c.identify()
    print("counters", want[2])
    assert want[2][0][1] < want[2][0][0] and want[2][4][1] > 0, want[2]      # passes skipped, fc1 rows listed
    assert c.prepared_launches() == 0
    c.prepare()
    assert c.identify() == want and c.prepared_launches() == 1 and c.seg.prepare_stats() == (1, 1)      # the call found its launches done
    assert c.identify() == want and c.seg.prepare_stats() == (1, 1)      # the record is gone: a whole chain again
    c.prepare(); c.prepare()
    assert c.identify() == want and c.prepared_launches() == 3 and c.seg.prepare_stats() == (3, 2)
    other = torch.from_numpy(np.ascontiguousarray(make_crops(6).reshape(N, -1))).cuda()
    c.prepare(d=other)
    assert c.identify() == want
    c.prepare(n=N - 40)
    assert c.identify() == want
    assert c.prepared_launches() == 5 and c.seg.prepare_stats() == (5, 2)      # neither mismatch was a hit
    small = c.identify(n=N - 40)
    c.prepare()
    assert c.identify(n=N - 40) == small                     # prepared for more crops than the call takes
    c.prepare()
    c.seg.load_weights(c.blob)
    assert c.identify() == want
    c.prepare()
    c.seg.set_identity_precision(capi.CNN_BF16X6)
    c.seg.set_identity_precision(capi.CNN_FP16X3)
    assert c.identify() == want
    assert c.seg.prepare_stats() == (8, 2)                   # (the call with n - 40 crops, the load and the precision change: no hits)
    c.seg.set_identity_precision(capi.CNN_BF16X6)
    n_before = c.prepared_launches()
    c.prepare()                                              # another mode has no such part
    assert c.prepared_launches() == n_before
    c.close()


def test_first_call_of_a_context_without_timers(monkeypatch, state, crops):
    """a context's first call is launched as it stands (function attributes are set there), timers or not"""
    a = Ctx(monkeypatch, state, RS, crops, timers=False)
    want = a.identify()
    a.close()
    b = Ctx(monkeypatch, state, RS, crops, timers=False)
    b.prepare()
    assert b.identify() == want
    b.close()


def test_a_prepare_that_is_never_consumed_in_front_of_a_replayed_graph(monkeypatch, state, crops):
    a = Ctx(monkeypatch, state, RS, crops, timers=False)
    want = [a.identify(n=100) for _ in range(4)]             # the fourth call replays the chain captured at the third
    a.close()
    b = Ctx(monkeypatch, state, RS, crops)
    b.prepare()
    assert b.prepared_launches() == 1
    b.seg.profile_enable(False)
    assert [b.identify(n=100) for _ in range(4)] == want
    b.prepare(n=100)                                         # the graph path: nothing is queued, nothing is remembered
    assert b.identify(n=100) == want[3]
    b.close()


@pytest.mark.parametrize("bit", range(21, 28))
def test_every_switch_of_the_chain(monkeypatch, state, crops, bit):
    c = Ctx(monkeypatch, state, RS | 1 << bit, crops)
    want = c.identify()
    c.prepare()
    assert c.identify() == want
    assert c.prepared_launches() == (0 if bit == 27 else 1)  # bit 27: no skipping, nothing to prepare
    c.close()


def test_background_out_of_the_fp16_range(monkeypatch, state, crops):
    """conv1's bias so large that the background itself leaves what two fp16 pieces hold (SK_EMPTY_RANGE set): every pass, pair and fc1 row is
    listed, and the guard re-runs"""
    st = {k: v.copy() for k, v in state.items()}
    st["bn1.bias"] = np.full(16, 6000.0, np.float32)
    st["bn2.running_var"] = np.full(64, 1e8, np.float32)
    c = Ctx(monkeypatch, st, RS, crops)
    want = c.identify()
    g = want[2][6]
    assert g[1] or g[0] > 0, g
    assert want[2][0][0] == want[2][0][1], want[2]            # every pass listed
    c.prepare()
    assert c.identify() == want and c.prepared_launches() == 1
    c.close()


def test_a_guard_tripping_crop(monkeypatch, state, crops):
    """conv1 scaled (with the statistics behind it) until bright noise leaves the fp16 range: the guard's re-run reads the crops again, behind a
    prepared pass as behind any other"""
    m = 65536.0
    st = {k: v.copy() for k, v in state.items()}
    st["conv1.weight"] *= m; st["conv1.bias"] *= m; st["bn1.running_mean"] *= m
    st["bn2.running_var"] = st["bn2.running_var"] * m * m
    dim = (crops >> 6).astype(np.uint8)                       # at most 3
    dim[5] = 255
    c = Ctx(monkeypatch, st, RS, dim)
    want = c.identify()
    g = want[2][6]
    print("guard", g)
    assert g[1] or g[0] > 0, g
    c.prepare()
    assert c.identify() == want and c.prepared_launches() == 1
    c.close()
