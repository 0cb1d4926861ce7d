"""The default 80 x 80 identity chain at the batch sizes that ship -- 25600 crops, a bench step, and the 32766 / 32767 crops around the largest
allocation from which every listed pass of conv3 still reaches an image of the empty crop -- with EVERY row of every call held to two expectations:

 1. float64.  Every crop of a batch is one of the 509 pool crops of tests/cnn_reach_cases.py; the float64 oracle (oracle/cnn_oracle.py) runs on
    the pool once, and row i of a call is held to the pool's row idx[i] with the bars of check_rows in test_cnn_trained_gpu.py: softmax within
    1e-4, row sums within 1e-5 of 1, logits within 8 x e32, e32 the largest distance of the fp32 oracle's logits from the float64 ones on the pool
    itself (measured here, printed, never taken from the device).
 2. bits.  The pool's 509 rows from ONE small call of the two-kernel chain (TREXHIP_CONV_GEOM bit 28) on a fresh context -- 5 MB of V3, no lists,
    no images, nothing skipped.  Row i of every large call equals row idx[i] of that call byte for byte, probabilities and logits: a row depends
    neither on its batch nor on the kernels its batch got.

What the large batches do that the tests of up to 12800 crops cannot (trex_amd/csrc/cnn_skip3.h, cnn_skip_kernels.h, net_forward_launch):
  * a listed pass bases its buffer resource at the front image while 20 + last row + 1 <= 393216 and at its own first row, reading the BACK
    image, from crop 19660 on; block 614 (crops 19648 .. 19679) straddles the switch;
  * V3 row 419430 (crop 20971) straddles byte 2^32 of V3: k_conv12_rs, k_v3_fill and both forms of k_conv5_wpair address past it;
  * the back image lies behind the ALLOCATION's rows: a context that served 32766 crops has it 655320 rows out when a 25600-crop call runs,
    and one that served 32767 keeps the copy in V3 although the call's plan says direct -- k_v3_fill and k_act3_fill must agree on that;
  * k_pair_count / k_pair_list run four workgroups of 8192 crops.
Which crop of a batch serves which of these, with the arithmetic: the docstring of tests/cnn_reach_cases.py; tests/test_cnn_reach_inputs.py
re-derives it on the CPU, and the counters asserted here (skip_stats, skip3_stats) are computed from the inputs there, not read off the device.

Measured figures (MI355X) are recorded in DESIGN.md section 4; the tests print them (run with -s).
"""
import functools
import numpy as np
import pytest
import torch

from oracle import cnn_oracle
from trex_amd import capi, weights
import cnn_reach_cases as rc

pytestmark = pytest.mark.gpu

COPY, DENSE3, NOSKIP, TWO = 1 << 25, 1 << 26, 1 << 27, 1 << 28
N_STEP, N_FITS, N_OUT = 25600, 32766, 32767      # a bench step; the largest allocation skip3_direct_fits takes (655320 <= 655335 rows); the first it does not
LOGIT_FACTOR = 8.0
CLASSES = 100


@functools.lru_cache(maxsize=None)
def state():
    return weights.synthetic_state(CLASSES, 31)


@functools.lru_cache(maxsize=None)
def float64_reference():
    """-> (softmax, logits) of the pool in float64, e32"""
    st, pool = state(), np.array(rc.pool())
    ps, ls, l32 = [], [], []
    for lo in range(0, len(pool), 128):
        p, l = cnn_oracle.predict(st, pool[lo:lo + 128], threads=16, dtype=torch.float64)
        ps.append(p); ls.append(l)
        l32.append(cnn_oracle.forward_logits(st, pool[lo:lo + 128], threads=16))
    p64, l64 = np.concatenate(ps), np.concatenate(ls)
    e32 = float(np.abs(np.concatenate(l32) - l64).max())
    print(f"pool: {len(pool)} crops, e32 = {e32:.3g}, max |logit| {np.abs(l64).max():.4g}, mean top softmax {p64.max(1).mean():.3f}")
    return p64, l64, e32


class Net:
    """a context with the synthetic weights loaded, in FP16X3; TREXHIP_CONV_GEOM is read when it is created"""

    def __init__(self, geom):
        with pytest.MonkeyPatch.context() as mp:
            if geom is None:
                mp.delenv("TREXHIP_CONV_GEOM", raising=False)
            else:
                mp.setenv("TREXHIP_CONV_GEOM", str(geom))
            self.seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
        self.seg.load_weights(weights.pack_blob(state(), CLASSES))
        self.seg.set_identity_precision(capi.CNN_FP16X3)

    def run(self, crops):
        """identify_device on torch buffers -> dict: probs, logits (float32 ndarrays), skip, skip3, guard"""
        n = len(crops)
        d = torch.from_numpy(np.ascontiguousarray(crops.reshape(n, -1))).cuda()
        probs = torch.full((n, CLASSES), -1.0, dtype=torch.float32, device="cuda")
        logits = torch.full_like(probs, -1.0)
        self.seg.identify_device(d.data_ptr(), n, probs.data_ptr(), logits.data_ptr())
        self.seg.synchronize()
        out = {"n": n, "probs": probs.cpu().numpy(), "logits": logits.cpu().numpy(), "skip": self.seg.skip_stats(), "skip3": self.seg.skip3_stats(),
               "guard": self.seg.guard_stats()}
        del d, probs, logits
        return out

    def close(self):
        self.seg.close()


@functools.lru_cache(maxsize=None)
def pool_bits():
    """expectation 2: the pool's rows from one 509-crop call of the two-kernel chain on a fresh context"""
    net = Net(TWO)
    out = net.run(np.array(rc.pool()))
    net.close()
    assert out["guard"] == (0, False)
    hold_float64("pool, two-kernel chain", out, np.arange(rc.P))
    return out["probs"], out["logits"]


def hold_float64(tag, out, idx, check=True):
    """expectation 1 on every row of a call; check=False: print the figures and return the assertions to make"""
    p64, l64, e32 = float64_reference()
    probs, logits = out["probs"], out["logits"]
    assert probs.shape == (len(idx), CLASSES) and np.all(np.isfinite(probs)) and np.all(np.isfinite(logits)), tag
    dp = float(np.abs(probs - p64[idx]).max())
    ds = float(np.abs(probs.astype(np.float64).sum(1) - 1.0).max())
    dl = float(np.abs(logits - l64[idx]).max())
    print(f"{tag}: n = {out['n']}, skip_stats {out['skip']}, skip3_stats {out['skip3']}, guard {out['guard']}; from float64: max |dp| {dp:.3g}, "
          f"max |row sum - 1| {ds:.3g}, max |dlogit| {dl:.3g} = {dl / e32:.3g} x e32 (e32 = {e32:.3g})")
    bars = [(dp <= 1e-4, (tag, "softmax", dp)), (ds <= 1e-5, (tag, "row sum", ds)), (dl <= LOGIT_FACTOR * e32, (tag, "logits", dl, e32))]
    if check:
        for ok, what in bars:
            assert ok, what
    return bars


def hold(tag, out, idx):
    """both expectations on every row of a call, and a quiet range guard"""
    bp, bl = pool_bits()
    bars = hold_float64(tag, out, idx, check=False)
    differ = (out["probs"].view(np.uint32) != bp[idx].view(np.uint32)).any(1) | (out["logits"].view(np.uint32) != bl[idx].view(np.uint32)).any(1)
    rows = np.flatnonzero(differ)
    print(f"{tag}: {len(rows)} of {len(idx)} rows differ in bits from the 509-crop two-kernel call" + (f", the first at crops {rows[:12].tolist()}" if len(rows) else ""))
    assert out["guard"] == (0, False), (tag, out["guard"])
    for ok, what in bars:
        assert ok, what
    assert len(rows) == 0, (tag, len(rows), rows[:12].tolist(), [int(idx[r]) for r in rows[:12]])


def hold_counters(tag, out, kind, skip3=True):
    """the device's counters against what the inputs say (cnn_reach_cases.expected_stats)"""
    e = rc.expected_stats(kind, out["n"])
    assert out["skip"] == e["skip"], (tag, out["skip"], e["skip"])
    if skip3:
        assert out["skip3"] == e["skip3"], (tag, out["skip3"], e["skip3"])


@functools.lru_cache(maxsize=None)
def sparse_step():
    """a fresh context of the default chain: S at 3200 crops -- the buffers grow and the images are placed anew behind it --, then S and S2 at 25600"""
    net = Net(None)
    outs = [net.run(rc.batch(kind, n)[0]) for kind, n in (("S", 3200), ("S", N_STEP), ("S2", N_STEP))]
    net.close()
    return outs


def test_bench_step_sparse():
    small, s, s2 = sparse_step()
    hold("S at 3200, fresh context", small, rc.indices("S", 3200))
    hold_counters("S at 3200", small, "S")
    for kind, out in (("S", s), ("S2", s2)):
        tag = f"{kind} at {N_STEP}"
        hold(tag, out, rc.indices(kind, N_STEP))
        pairs, listed, passes, filled = out["skip3"]
        assert pairs == 256000 and 0 < listed < pairs and passes > 0 and filled == (pairs - listed) * 5120, (tag, out["skip3"])
        assert out["skip"][1] < out["skip"][0], (tag, out["skip"])
        hold_counters(tag, out, kind)
    assert s["skip3"] != s2["skip3"]


def test_bench_step_noise_and_mixed():
    net = Net(None)
    noise = net.run(rc.batch("N", N_STEP)[0])
    mixed = net.run(rc.batch("M", N_STEP)[0])
    net.close()
    hold(f"N at {N_STEP}", noise, rc.indices("N", N_STEP))
    assert noise["skip3"][:3] == (256000, 256000, 0), noise["skip3"]
    hold_counters("N", noise, "N")
    hold(f"M at {N_STEP}, behind N", mixed, rc.indices("M", N_STEP))
    assert mixed["skip3"][2] == 0 and mixed["skip"][2] > 0, (mixed["skip3"], mixed["skip"])
    hold_counters("M", mixed, "M")


def test_back_image_at_the_limit_of_reach():
    """noise at 32766 crops leaves noise-derived bits in every V3 row; the sparse batches behind it compute their own rows only and read the
    rest from the images -- the back one behind 655320 rows for the 25600-crop call as well"""
    net = Net(None)
    noise = net.run(rc.batch("N", N_FITS)[0])
    big = net.run(rc.batch("S", N_FITS)[0])
    step = net.run(rc.batch("S", N_STEP)[0])
    net.close()
    hold(f"N at {N_FITS}", noise, rc.indices("N", N_FITS))
    hold_counters("N", noise, "N")
    hold(f"S at {N_FITS}, behind N", big, rc.indices("S", N_FITS))
    assert big["skip3"][2] > 0
    hold_counters("S", big, "S")
    hold(f"S at {N_STEP}, in the buffers of {N_FITS}", step, rc.indices("S", N_STEP))
    assert step["skip3"][2] > 0
    hold_counters("S", step, "S")
    first = sparse_step()[1]
    assert step["probs"].tobytes() == first["probs"].tobytes() and step["logits"].tobytes() == first["logits"].tobytes()
    assert step["skip"] == first["skip"] and step["skip3"] == first["skip3"]


def test_allocation_out_of_reach_keeps_the_copy():
    """655340 rows of allocation: out of both images' reach in the middle.  The 25600-crop call's plan says direct, the allocation says no: the
    fill must copy and the listed passes must read the copy, over the noise of the call before"""
    net = Net(None)
    noise = net.run(rc.batch("N", N_OUT)[0])
    step = net.run(rc.batch("S", N_STEP)[0])
    net.close()
    hold(f"N at {N_OUT}", noise, rc.indices("N", N_OUT))
    hold_counters("N", noise, "N")
    hold(f"S at {N_STEP}, in the buffers of {N_OUT}", step, rc.indices("S", N_STEP))
    assert step["skip3"][2] > 0, step["skip3"]
    hold_counters("S", step, "S")


@pytest.mark.parametrize("geom,name", [(COPY, "bit 25, the copy kept"), (DENSE3, "bit 26, dense conv3"), (NOSKIP, "bit 27, nothing skipped")])
def test_forced_forms_agree_at_the_bench_step(geom, name):
    """the copy past 4 GB, and the dense kernels past 4 GB on sparse crops"""
    net = Net(geom)
    out = net.run(rc.batch("S", N_STEP)[0])
    net.close()
    hold(f"S at {N_STEP}, {name}", out, rc.indices("S", N_STEP))
    if geom == COPY:
        assert out["skip3"][2] > 0
        hold_counters(name, out, "S")
    if geom == DENSE3:
        hold_counters(name, out, "S", skip3=False)
