"""The yardsticks of the v100 / v110 training step, on the CPU:
  1. the float64 restatement (tests/train_arch_ref.py) reproduces what the reference's own modules + torch.optim.Adam produced
     (tests/golden/cnn_train_arch.npz, generator tests/golden/make_train_arch_fixture.py) within the bars the device is held to;
  2. at every case of tests/train_arch_cases.py the float32 restatement stays within a fifth of each bar of the float64 one, so a miss on the
     device is the device's;
  3. what each case reaches, by arithmetic on the table."""
import os
import numpy as np
import pytest
import torch

import train_arch_cases as tc
import train_arch_ref as ref

FIX = os.path.join(os.path.dirname(__file__), "golden", "cnn_train_arch.npz")
SAMPLE = {"conv2.weight": 7, "conv3.weight": 23, "fc1.weight": 11}


def sample(name, arr):
    return np.asarray(arr).reshape(-1)[::SAMPLE.get(name, 1)]


@pytest.mark.parametrize("name", ["v100_c1", "v100_c3", "v110_c1", "v110_c3"])
def test_the_float64_restatement_reproduces_the_reference(name):
    fx = np.load(FIX)
    arch = name.split("_")[0]
    W, H, ch, n, classes, steps, seed = [int(v) for v in fx[f"{name}/meta"]]
    lr = float(fx[f"{name}/lr"][0])
    case = ((W, H, ch, n, classes), seed, "fixture")
    state = tc.initial_state(case, arch)
    adam = ref.new_adam_state(arch, state)
    zero = ref.zero_gradient(arch)
    for s in range(steps):
        x, y, masks = tc.inputs(case, arch, s)
        for t in masks:
            assert np.array_equal(masks[t].astype(np.uint8), fx[f"{name}/mask{s}/{t}"]), (s, t)
        state, loss, correct, grads = ref.train_step(arch, state, adam, x, y, masks, lr, dtype=torch.float64)
        want = float(fx[f"{name}/loss{s}"][0])
        assert abs(loss - want) <= 5e-5 * max(1.0, abs(want)), (s, loss, want)
        assert correct == int(fx[f"{name}/correct{s}"][0])
        if s == 0:
            for k in ref.trainable(arch):
                r, got = fx[f"{name}/grad0/{k}"], sample(k, grads[k])
                if k in zero:
                    assert max(np.abs(got).max(), np.abs(r).max()) <= 1e-4 * max(1.0, float(np.abs(fx[f"{name}/grad0/{zero[k]}"]).max())), k
                else:
                    assert np.abs(got - r).max() <= tc.GRAD_RTOL * float(np.abs(r).max()), (k, float(np.abs(got - r).max()))
    for k in ref.trainable(arch) + ref.buffers(arch):
        r, got = fx[f"{name}/final/{k}"], sample(k, state[k])
        err = np.abs(got - r)
        assert err.max() <= 1e-4 * max(1.0, float(np.abs(r).max())), (k, float(err.max()))
        if k in ref.trainable(arch) and k not in zero:      # Adam's +-lr per step on rounding noise aside, the chains agree far inside lr
            assert np.mean(err <= 0.05 * lr + 1e-6 * np.abs(r)) >= 0.99, (k, float(np.mean(err <= 0.05 * lr + 1e-6 * np.abs(r))))


@pytest.mark.parametrize("arch", tc.ARCHS)
@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_float32_stays_within_a_fifth_of_every_bar_of_float64(case, arch):
    m = tc.margins(case, arch)
    worst = max(m, key=m.get)
    print(f"{tc.case_id(case)} {arch}: worst fraction of its bar {m[worst]:.3g} ({worst})")
    assert m[worst] <= 0.2, (worst, m[worst])
    assert case[0][3] >= 3                                     # BatchNorm over two values is ill-conditioned


def shares(rows, max_shares):
    s = min(rows, max_shares)
    per = -(-rows // s)
    return per, -(-rows // per), rows % per != 0


def test_what_each_case_reaches():
    """by arithmetic on the table (train_geom.h's rules: floors per level, 64-window tiles, 64-column strips of 8 rows, at most 96 / 48 shares)"""
    by = {c[0][:2]: c[0] for c in tc.CASES}
    assert len(by) == len(tc.CASES) == 8
    lv = {k: tc.levels(*k) for k in by}
    # the pooled plane in front of fc1 is 1 x 1: block 3's BatchNorm2d counts n values
    assert lv[(8, 8)][3] == (1, 1) and by[(8, 8)][3] == 3
    # an odd conv1 plane on one axis only, three channels
    assert lv[(9, 8)][0] == (9, 8) and lv[(9, 8)][1] == (4, 4) and by[(9, 8)][2] == 3
    # odd planes at blocks 2 and 3 on either axis, both orientations, 100 classes on one
    assert lv[(21, 13)] == [(21, 13), (10, 6), (5, 3), (2, 1)] and lv[(13, 21)] == [(13, 21), (6, 10), (3, 5), (1, 2)]
    assert by[(21, 13)][4] == 100 and by[(21, 13)][2] == 3 and by[(13, 21)][2] == 1
    # an odd plane at block 3 only
    assert lv[(44, 28)][:3] == [(44, 28), (22, 14), (11, 7)]
    assert (80, 80) in by
    # several tiles: more than 64 windows in conv2's and conv3's planes; a second wgrad1 strip (W > 64); ragged weight-gradient shares
    windows = {k: [((w + 1) // 2) * ((h + 1) // 2) for w, h in lv[k][1:3]] for k in by}
    assert windows[(100, 60)] == [375, 104] and windows[(14, 100)] == [100, 26]      # conv2, conv3: 64 windows per tile
    assert all(max(windows[k]) <= 64 for k in ((8, 8), (9, 8), (21, 13), (13, 21)))
    assert -(-100 // 64) == 2 and 60 % 8 != 0
    n = by[(100, 60)][3]
    assert shares(n * lv[(100, 60)][1][1], 96) == (1, 90, False) and shares(n * lv[(100, 60)][2][1], 48) == (1, 45, False)
    n = by[(14, 100)][3]
    assert shares(n * lv[(14, 100)][1][1], 96) == (3, 84, True) and shares(n * lv[(14, 100)][2][1], 48) == (3, 42, True)
    # every case holds a dropped channel in some plane of both versions' masks and keeps most
    for case in tc.CASES:
        for arch in tc.ARCHS:
            _, _, masks = tc.inputs(case, arch)
            assert any((~m).any() for m in masks.values()) and all(m.mean() > 0.3 for m in masks.values()), (tc.case_id(case), arch)
