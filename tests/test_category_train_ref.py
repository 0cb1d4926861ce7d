"""The yardsticks of the category network's training step, on the CPU:
  1. the float64 restatement (tests/category_train_ref.py) reproduces what the reference's own module + torch.optim.Adam produced
     (tests/golden/category_train.npz, generator tests/golden/make_category_train_fixture.py) within the bars the device is held to;
  2. at every case of tests/category_train_cases.py the float32 restatement stays within a fifth of each bar of the float64 one, so a miss on the
     device is the device's;
  3. what each case reaches, by arithmetic on the table;
  4. the two wrong first layers -- padding staged as -1, the offset folded into the bias -- miss conv1.weight's gradient by orders of magnitude on
     the border batch of the device test, so that test can see them;
  5. the mask layout the ABI states, and the way back of tools/convert_category_weights.py."""
import os
import subprocess
import sys
import numpy as np
import pytest
import torch

from trex_amd import weights
import category_train_cases as tc
import category_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(os.path.dirname(__file__), "golden", "category_train.npz")
SAMPLE = {"conv2.weight": 3, "conv3.weight": 11, "fc1.weight": 7}


def sample(name, arr):
    return np.asarray(arr).reshape(-1)[::SAMPLE.get(name, 1)]


@pytest.mark.parametrize("name", ["c1", "c3"])
def test_the_float64_restatement_reproduces_the_reference(name):
    fx = np.load(FIX)
    W, H, ch, n, categories, steps, seed = [int(v) for v in fx[f"{name}/meta"]]
    lr = float(fx[f"{name}/lr"][0])
    case = ((W, H, ch, n, categories), seed, "fixture")
    chain = ref.Chain(tc.initial_state(case), lr, dtype=torch.float64)
    for s in range(steps):
        x, y, masks = tc.inputs(case, s)
        for t in masks:
            assert np.array_equal(np.packbits(masks[t].astype(np.uint8).reshape(-1)), fx[f"{name}/mask{s}/{t}"]), (s, t)
        loss, correct, grads = chain.step(x, y, masks)
        want = float(fx[f"{name}/loss{s}"][0])
        assert abs(loss - want) <= 5e-5 * max(1.0, abs(want)), (s, loss, want)
        assert correct == int(fx[f"{name}/correct{s}"][0])
        if s == 0:
            for k in ref.trainable():
                r, got = fx[f"{name}/grad0/{k}"], sample(k, grads[k])
                if k in tc.ZERO_GRADIENT:
                    assert max(np.abs(got).max(), np.abs(r).max()) <= 1e-4 * max(1.0, float(np.abs(fx[f"{name}/grad0/{tc.ZERO_GRADIENT[k]}"]).max())), k
                else:
                    assert np.abs(got - r).max() <= tc.GRAD_RTOL * float(np.abs(r).max()), (k, float(np.abs(got - r).max()))
    state = chain.state()
    assert len(state) == 22
    for k in ref.trainable() + ref.buffers():
        r, got = fx[f"{name}/final/{k}"], sample(k, state[k])
        err = np.abs(got - r)
        assert err.max() <= 1e-4 * max(1.0, float(np.abs(r).max())), (k, float(err.max()))


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_float32_stays_within_a_fifth_of_every_bar_of_float64(case):
    m = tc.margins(case)
    worst = max(m, key=m.get)
    print(f"{tc.case_id(case)}: worst fraction of its bar {m[worst]:.3g} ({worst})")
    assert m[worst] <= 0.2, (worst, m[worst])
    W, H = case[0][:2]
    assert case[1] == 3000 + 7 * W + H                         # the first seed of the rule passes at every case


def shares(rows, max_shares):
    s = min(rows, max_shares)
    per = -(-rows // s)
    return per, -(-rows // per), rows % per != 0


def test_what_each_case_reaches():
    by = {c[0][:2]: c[0] for c in tc.CASES}
    assert len(by) == len(tc.CASES) == 9
    planes = {k: [(k[1], k[0])] + ref.pooled_planes(*k) for k in by}        # (h, w) of z1, z2, z3 and of fc1's input
    assert planes[(8, 8)][2:] == [(2, 2), (1, 1)] and by[(8, 8)][3] == 3
    assert planes[(9, 8)][:2] == [(8, 9), (4, 4)] and by[(9, 8)][2] == 3
    assert planes[(21, 13)] == [(13, 21), (6, 10), (3, 5), (1, 2)] and by[(21, 13)][4] == 70 and by[(21, 13)][2] == 3
    assert planes[(13, 21)] == [(21, 13), (10, 6), (5, 3), (2, 1)] and by[(13, 21)][2] == 1
    assert [s for s in by.values() if s[3] == 1] == [by[(24, 16)]]
    # conv2's plane at 80 x 80 is 40 x 40: 20 x 20 windows = 3 x 3 tiles of 8 x 8
    assert planes[(80, 80)][1] == (40, 40) and -(-20 // 8) == 3
    # 100 x 60: ragged tiles both ways (25 x 15 windows of conv2), a second 64-column strip and a ragged 8-row band of k_tany_wgrad1
    assert planes[(100, 60)][1] == (30, 50) and 25 % 8 and 15 % 8 and -(-100 // 64) == 2 and 60 % 8 != 0 and by[(100, 60)][2] == 3
    # 14 x 100: conv2's plane is 7 wide = 4 windows; the shares of both weight gradients straddle crops
    n = by[(14, 100)][3]
    assert planes[(14, 100)][1] == (50, 7) and shares(n * 50, 96) == (3, 84, True) and shares(n * 25, 48) == (3, 42, True)
    # 100 x 14: conv2's plane is 50 wide = 25 windows and 4 windows high
    assert planes[(100, 14)][1] == (7, 50)
    for case in tc.CASES:                                        # every plane of every case drops some elements and keeps most
        _, _, masks = tc.inputs(case)
        assert all((~m).any() and m.mean() > 0.5 for m in masks.values()), tc.case_id(case)
        st = tc.initial_state(case)
        for i in (1, 2, 3):
            g = st[f"batch_norm{i}.weight"]
            assert 0.25 <= (g < 0).mean() <= 0.4 and not np.allclose(st[f"batch_norm{i}.running_var"], 1)
        w = st["conv2.weight"]
        assert not np.allclose(w, w[:, :, ::-1, ::-1])            # no symmetric kernels: an unflipped data gradient shows


def border_batch(case):
    """the batch of the normalisation / padding check: the border pixels are byte 0 (normalised -1, where a wrong padding value changes most) and
    conv1's weights are large at the border taps"""
    x, y, masks = tc.inputs(case)
    x = x.copy()
    x[:, 0, :, :] = 0; x[:, -1, :, :] = 0; x[:, :, 0, :] = 0; x[:, :, -1, :] = 0
    st = dict(tc.initial_state(case))
    w = st["conv1.weight"].copy()
    w[:, :, 0, :] *= 4; w[:, :, 2, :] *= 4; w[:, :, :, 0] *= 4; w[:, :, :, 2] *= 4
    st["conv1.weight"] = w
    return st, x, y, masks


def test_the_wrong_first_layers_miss_by_orders_of_magnitude():
    case = tc.find(9, 8)
    st, x, y, masks = border_batch(case)
    _, _, g64, _ = ref.forward_backward(st, x, y, masks, dtype=torch.float64)
    _, _, g32, _ = ref.forward_backward(st, x, y, masks, dtype=torch.float32)
    err, bar = tc.gradient_error("conv1.weight", g32, g64)
    assert err <= 0.2 * bar
    for mutant in ("pad_minus_one", "offset_in_bias"):
        _, _, gm, _ = ref.forward_backward(st, x, y, masks, dtype=torch.float64, mutant=mutant)
        err, bar = tc.gradient_error("conv1.weight", gm, g64)
        print(f"{mutant}: conv1.weight gradient {err / bar:.3g} of the bar")
        assert err >= 100 * bar, (mutant, err, bar)


def test_the_mask_layout():
    assert ref.mask_shapes(2, 21, 13) == [("d1", (2, 6, 10, 16)), ("d2", (2, 3, 5, 64)), ("d3", (2, 1, 2, 100)), ("d4", (2, 100))]
    assert ref.mask_bytes(2, 21, 13) == 2 * (6 * 10 * 16 + 3 * 5 * 64 + 1 * 2 * 100 + 100)
    m = ref.draw_masks(2, 21, 13, 1)
    assert ref.pack_masks(m).shape == (ref.mask_bytes(2, 21, 13),) and set(np.unique(ref.pack_masks(m))) == {0, 1}


def test_the_converter_goes_both_ways(tmp_path):
    st = weights.synthetic_category_state(3, 5, channels=3, width=16, height=24)
    blob = weights.pack_category_blob(st, 3, 3, 16, 24)
    src, out = tmp_path / "in.trxc", tmp_path / "out.pth"
    src.write_bytes(blob)
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "convert_category_weights.py"), "--from-blob", str(src), str(out)])
    ck = torch.load(str(out), map_location="cpu", weights_only=True)
    assert list(ck["model_state"]) == [n for n, _ in weights.category_shapes(3, 3, 16, 24)]
    back = {k: v.numpy() for k, v in ck["model_state"].items()}
    assert weights.pack_category_blob(back, 3, 3, 16, 24) == blob
