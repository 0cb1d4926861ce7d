"""The architecture chains (cnn_arch.hip) at the shapes, class counts and call sizes where their kernels take another path, against float64
(tests/vi_arch_ref.py).  The cases are tests/cnn_arch_edge_cases.py; what each of them reaches is shown from the plan, on the CPU, by
test_cnn_arch_plan.py.  The rule is test_cnn_arch_gpu.py's, unchanged: logits within LOGIT_FACTOR x e32 of float64, e32 the float32
restatement's own error on the same crops; the arg-max equal on decided rows; at most UNDECIDED_CAP undecided.

  1. every case of the table in every mode, the device route and the host route
  2. a call past ARCH_CHUNK_MAX crops: the second chunk's offsets
  3. the range guard: loud crops in both chunks of a call, several listed crops (v110, v119, v200)
  4. more than FB_MAX loud crops: the whole-chunk re-run, the state it leaves, a call that mixes both kinds of chunk"""
import numpy as np
import pytest
import torch
from trex_amd import capi, weights
import vi_arch_ref
from cnn_arch_edge_cases import CASES, case_id, make
from test_cnn_arch_gpu import EXACT_MODES, LOGIT_FACTOR, UNDECIDED_CAP, _first_layer_max, make_net, run_device

pytestmark = pytest.mark.gpu

CHUNK_MAX = 1 << 16          # ARCH_CHUNK_MAX (cnn_arch_plan.h)
FB_MAX = 1024                # cnn_geom.h
MODE_NAMES = {capi.CNN_FP32: "FP32", capi.CNN_BF16X6: "BF16X6", capi.CNN_BF16X3: "BF16X3", capi.CNN_FP16X3: "FP16X3"}


def reference(st, crops, arch):
    """-> (float64 softmax, float64 logits, e32, decided rows), the undecided share asserted"""
    p64, l64 = vi_arch_ref.forward(st, crops, arch, torch.float64, threads=16)
    _, l32 = vi_arch_ref.forward(st, crops, arch, torch.float32, threads=16)
    e32 = float(np.abs(l32 - l64).max())
    if l64.shape[1] == 1:
        decided = np.ones(l64.shape[0], bool)
    else:
        top = np.sort(l64, 1)
        decided = (top[:, -1] - top[:, -2]) > 2 * LOGIT_FACTOR * e32
    assert e32 > 0 and (~decided).mean() <= UNDECIDED_CAP, (e32, int((~decided).sum()))
    return p64, l64, e32, decided


def hold(tag, lg, l64, e32, decided):
    """the float64 rule on logits"""
    ratio = float(np.abs(lg - l64).max()) / e32
    print(f"{tag}: max |dlogit| = {ratio:.3g} x e32 (e32 = {e32:.3g}), undecided {int((~decided).sum())} of {len(decided)}")
    assert np.all(np.isfinite(lg)) and ratio <= LOGIT_FACTOR, (tag, ratio, e32)
    assert np.array_equal(lg.argmax(1)[decided], l64.argmax(1)[decided]), tag
    return ratio


# ---- 1. float64 at every case of the table ----
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_case_against_float64(case):
    arch, w, h, ch, classes, n, _, _ = case
    st, crops = make(case)
    p64, l64, e32, decided = reference(st, crops, arch)
    seg = make_net(st, classes, ch, w, h, arch)
    assert seg.identify_chunk_crops() >= n
    for mode in [capi.CNN_BF16X3] + EXACT_MODES:          # (FP16X3 last, as in test_cnn_arch_gpu.py)
        seg.set_identity_precision(mode)
        p, lg = run_device(seg, crops, classes)
        host = seg.probabilities(crops)
        assert p.shape == (n, classes) and np.all(np.isfinite(p)) and np.all(np.isfinite(lg))
        assert np.abs(host - p).max() <= 1e-6
        assert np.allclose(p.sum(1), 1.0, atol=1e-5)
        if classes == 1:
            assert np.all(p == 1.0)
        if mode == capi.CNN_BF16X3:                        # three piece products: finite and normalised, not held to the bar
            continue
        hold(f"{case_id(case)} {MODE_NAMES[mode]}", lg, l64, e32, decided)
        assert np.abs(p - p64).max() <= 1e-4, (mode, np.abs(p - p64).max())
        if mode == capi.CNN_FP16X3:
            assert seg.guard_stats() == (0, False)
    seg.close()


# ---- the small v110 net of the call-size tests: 8x8, where a chunk is ARCH_CHUNK_MAX crops ----
def small_net(arch="v110", w=8, h=8, seed=41):
    return {k: v.copy() for k, v in weights.synthetic_state(8, seed, 1, w, h, arch=arch).items()}


def sample_rows(n, fixed, seed=7, extra=256):
    rows = set(fixed) | set(np.random.default_rng(seed).choice(n, extra, replace=False).tolist())
    return np.array(sorted(rows))


# ---- 2. past ARCH_CHUNK_MAX ----
def test_a_call_past_the_chunk_cap():
    arch, n = "v110", CHUNK_MAX + 3
    st = small_net(arch)
    crops = np.random.default_rng(42).integers(0, 256, (n, 8, 8, 1), dtype=np.uint8)
    rows = sample_rows(n, [0, CHUNK_MAX - 1, CHUNK_MAX, n - 1])
    p64, l64, e32, decided = reference(st, crops[rows], arch)
    seg = make_net(st, 8, 1, 8, 8, arch)
    assert seg.identify_chunk_crops() == CHUNK_MAX
    for mode in EXACT_MODES:
        seg.set_identity_precision(mode)
        p, lg = run_device(seg, crops, 8)
        if mode == capi.CNN_FP16X3:
            assert seg.guard_stats() == (0, False)
        pa, lga = run_device(seg, crops[:CHUNK_MAX], 8)
        pb, lgb = run_device(seg, crops[CHUNK_MAX:], 8)
        for one, two, what in ((p, np.concatenate([pa, pb]), "softmax"), (lg, np.concatenate([lga, lgb]), "logits")):
            differ = np.flatnonzero((one.view(np.uint32) != two.view(np.uint32)).any(1))
            assert differ.size == 0, (mode, what, differ[:8])
        hold(f"past the cap {MODE_NAMES[mode]}", lg[rows], l64, e32, decided)
        assert np.abs(p[rows] - p64).max() <= 1e-4
        assert np.all(np.isfinite(p)) and np.allclose(p.sum(1), 1.0, atol=1e-5)
    seg.close()


# ---- 3. / 4. the range guard ----
def loud_net(arch, w, h, quiet, loud_crops, seed=41):
    """the BatchNorm scaling of test_range_guard_reruns_only_the_loud_crop: the first layer's output times m, so that every quiet crop peaks at
    3000 and every loud one beyond the fp16 range, and the scale taken back behind the second convolution"""
    st = small_net(arch, w, h, seed)
    base_q = _first_layer_max(st, quiet, arch).max()
    base_l = _first_layer_max(st, loud_crops, arch).min()
    m = 3000.0 / max(base_q, 1e-9)
    assert base_l * m > 2 * 65520, (base_q, base_l)
    st["bn1.weight"] *= m; st["bn1.bias"] *= m
    st["bn2.running_var"] = st["bn2.running_var"] * m * m
    st["bn2.running_mean"] = st["bn2.running_mean"] * m
    st["conv2.bias"] *= m
    return st


def quiet_and_loud(n, w, h, loud, seed):
    """n quiet crops (values 0..3 in the middle half) and the same with the rows `loud` replaced by full-range noise"""
    rng = np.random.default_rng(seed)
    quiet = np.zeros((n, h, w, 1), np.uint8)
    quiet[:, h // 4:h - h // 4, w // 4:w - w // 4, 0] = rng.integers(0, 4, (n, h - 2 * (h // 4), w - 2 * (w // 4)))
    crops = quiet.copy()
    crops[loud] = rng.integers(128, 256, (len(loud), h, w, 1))
    return quiet, crops


def check_listed(seg, st, arch, quiet, crops, loud, rows):
    """FP16X3 on `crops`: exactly the loud rows are re-run and right, every other row is the bits of the run on quiet crops; the logits of
    `rows` (the loud ones among them, at least 64 rows of 8 classes) by the float64 rule"""
    n = crops.shape[0]
    assert set(loud) <= set(rows.tolist()) and len(rows) >= 64
    _, l64, e32, decided = reference(st, crops[rows], arch)
    seg.set_identity_precision(capi.CNN_FP16X3)
    pq, lq = run_device(seg, quiet, 8)
    assert seg.guard_stats() == (0, False)
    p, lg = run_device(seg, crops, 8)
    assert seg.guard_stats() == (len(loud), False)
    seg.set_identity_precision(capi.CNN_FP32)
    exact, _ = run_device(seg, crops[loud], 8)
    ref, _ = vi_arch_ref.forward(st, crops[loud], arch, torch.float64)
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(lg))
    print(arch, "loud rows: vs FP32", np.abs(p[loud] - exact).max(axis=1), "vs float64", np.abs(p[loud] - ref).max(axis=1))
    assert np.abs(p[loud] - exact).max() <= 1e-4 and np.abs(p[loud] - ref).max() <= 1e-4
    others = np.ones(n, bool); others[loud] = False
    differ = np.flatnonzero(others & ((p.view(np.uint32) != pq.view(np.uint32)).any(1) | (lg.view(np.uint32) != lq.view(np.uint32)).any(1)))
    assert differ.size == 0, differ[:8]
    hold(f"{arch} guarded call, {len(loud)} rows re-run in BF16X6", lg[rows], l64, e32, decided)      # (the softmax of these nets saturates: the logits say more)


def test_range_guard_across_chunks():
    arch, n = "v110", CHUNK_MAX + 3
    loud = [0, 5, 6, 1999, CHUNK_MAX - 1, CHUNK_MAX, n - 1]        # both chunks, adjacent and not, both sides of the boundary
    quiet, crops = quiet_and_loud(n, 8, 8, loud, 43)
    st = loud_net(arch, 8, 8, quiet, crops[loud])
    seg = make_net(st, 8, 1, 8, 8, arch)
    assert seg.identify_chunk_crops() == CHUNK_MAX
    check_listed(seg, st, arch, quiet, crops, loud, sample_rows(n, loud))
    seg.close()


@pytest.mark.parametrize("arch,w,h", [("v200", 55, 29), ("v119", 33, 17)])
def test_range_guard_lists_several_crops(arch, w, h):
    n, loud = 64, [0, 3, 4, 17, 63]
    quiet, crops = quiet_and_loud(n, w, h, loud, 44)
    st = loud_net(arch, w, h, quiet, crops[loud])
    seg = make_net(st, 8, 1, w, h, arch)
    assert seg.identify_chunk_crops() >= n
    check_listed(seg, st, arch, quiet, crops, loud, np.arange(n))
    seg.close()


def test_whole_chunk_rerun_and_the_state_it_leaves():
    arch, n, k = "v110", 1200, 1100
    assert k > FB_MAX
    loud = np.sort(np.random.default_rng(45).choice(n, k, replace=False))
    quiet, crops = quiet_and_loud(n, 8, 8, loud, 46)
    st = loud_net(arch, 8, 8, quiet, crops[loud])
    fresh = make_net(st, 8, 1, 8, 8, arch)
    pq, lq = run_device(fresh, quiet, 8)                 # FP16X3, the default
    assert fresh.guard_stats() == (0, False)
    fresh.close()
    seg = make_net(st, 8, 1, 8, 8, arch)
    p, lg = run_device(seg, crops, 8)
    assert seg.guard_stats() == (0, True)                # k_arch_guard_plan: a whole chunk adds nothing to the first word
    ref, l64, e32, decided = reference(st, crops, arch)
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(lg))
    print("whole chunk: max |dp| vs float64", np.abs(p - ref).max())
    assert np.abs(p - ref).max() <= 1e-4
    hold("whole chunk, re-run in BF16X6", lg, l64, e32, decided)          # (the softmax of these nets saturates: the logits say more)
    p2, lg2 = run_device(seg, quiet, 8)                  # flags, plan and range word were cleared
    assert seg.guard_stats() == (0, False)
    assert p2.tobytes() == pq.tobytes() and lg2.tobytes() == lq.tobytes()
    seg.close()


@pytest.mark.parametrize("whole_first", [True, False])
def test_a_call_with_a_listed_and_a_whole_chunk(whole_first):
    arch, k = "v110", 1100
    tail = 1200
    n = CHUNK_MAX + tail
    rng = np.random.default_rng(47)
    listed = np.array([1, 2, 700]) + (CHUNK_MAX if whole_first else 0)
    many = np.sort(rng.choice(CHUNK_MAX if whole_first else tail, k, replace=False)) + (0 if whole_first else CHUNK_MAX)
    loud = np.sort(np.concatenate([listed, many]))
    quiet, crops = quiet_and_loud(n, 8, 8, loud, 48)
    st = loud_net(arch, 8, 8, quiet, crops[loud])
    seg = make_net(st, 8, 1, 8, 8, arch)
    pq, lq = run_device(seg, quiet, 8)
    assert seg.guard_stats() == (0, False)
    p, lg = run_device(seg, crops, 8)
    assert seg.guard_stats() == (len(listed), True)      # the listed chunk's crops in the first word, the whole chunk in the second
    assert np.all(np.isfinite(p)) and np.all(np.isfinite(lg))
    in_listed = np.arange(n) >= CHUNK_MAX if whole_first else np.arange(n) < CHUNK_MAX
    others = in_listed.copy(); others[listed] = False    # quiet rows of the listed chunk: the bits of the quiet run
    differ = np.flatnonzero(others & ((p.view(np.uint32) != pq.view(np.uint32)).any(1) | (lg.view(np.uint32) != lq.view(np.uint32)).any(1)))
    assert differ.size == 0, differ[:8]
    rows = sample_rows(n, loud.tolist() + [0, CHUNK_MAX - 1, CHUNK_MAX, n - 1], seed=49)
    ref, l64, e32, decided = reference(st, crops[rows], arch)
    print("mixed call: max |dp| vs float64", np.abs(p[rows] - ref).max())
    assert np.abs(p[rows] - ref).max() <= 1e-4
    hold("mixed call", lg[rows], l64, e32, decided)
    seg.close()
