"""The category network and the tracklet vote on the CPU: the restatement (tests/category_ref.py) against the reference's own vectors
(tests/golden/category.npz, written by make_category_fixture.py from the reference's PyTorchModel), what the case table reaches, the float64 margin
of every chosen input, the padding clause, the blob and its converter, and hand cases of the vote and of sample_rows."""
import os
import subprocess
import sys
import numpy as np
import pytest
import torch
from trex_amd import weights
import category_cases as cc
import category_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import convert_category_weights as conv  # noqa: E402


def test_fixture_is_small_and_complete():
    assert os.path.getsize(cc.FIXTURE) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "cnn_train_arch.npz"))
    fx = cc.fixture()
    for case in cc.CASES:
        pre = f"case/{cc.case_id(case)}/"
        assert sorted(k[len(pre):] for k in fx if k.startswith(pre)) == sorted(
            [f"stat/batch_norm{i}.running_{s}" for i in (1, 2, 3) for s in ("mean", "var")] + [f"{k}/{n}" for k in ("logits", "probs", "labels") for n in cc.BATCHES])
    assert sorted({c[0][3] for c in cc.CASES}) == [2, 3, 5, 70, 1024] and {c[0][2] for c in cc.CASES} == {1, 3}


def test_the_normalisation_is_a_true_division():
    # what the kernel's comment states: torch's float32 `x / 127.5 - 1` is a division and a subtraction, each rounded on its own, for every byte
    b = np.arange(256, dtype=np.uint8)
    want = (torch.tensor(b.astype(np.float32)) / 127.5 - 1).numpy().view(np.uint32)
    x = b.astype(np.float32)
    div = (x / np.float32(127.5) - np.float32(1)).view(np.uint32)
    r = np.float32(1) / np.float32(127.5)
    mul = (x * r - np.float32(1)).view(np.uint32)
    fused = (x.astype(np.float64) * np.float64(r) - 1).astype(np.float32).view(np.uint32)      # one rounding: a fused multiply-subtract
    assert np.array_equal(div, want)
    assert int((mul != want).sum()) == 111 and int((fused != want).sum()) == 205
    assert np.array_equal(cr.normalise(b.reshape(1, 16, 16, 1)).numpy().reshape(-1).view(np.uint32), want)


@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_restatement_against_the_reference_and_float64(case):
    (w, h, ch, cats), seed, _ = case
    assert seed == 3000 + 7 * w + h                                 # the first candidate held at every case
    st, fx, pre = cc.state(case), cc.fixture(), f"case/{cc.case_id(case)}/"
    for n in cc.BATCHES:
        crops = cc.crops(case, n)
        assert crops.shape == (n, h, w, ch) and crops.min() < 40 and crops.max() > 215
        edge = np.concatenate([crops[:, 0].ravel(), crops[:, -1].ravel(), crops[:, :, 0].ravel(), crops[:, :, -1].ravel()])
        assert edge.std() > 30                                      # textured to the crop's edge
        p32, l32, lab32 = cr.forward(st, crops, torch.float32)
        p64, l64, lab64 = cr.forward(st, crops, torch.float64)
        dp, dl = float(np.abs(p32 - fx[pre + f"probs/{n}"]).max()), float(np.abs(l32 - fx[pre + f"logits/{n}"]).max())
        e32 = float(np.abs(l32 - l64).max())
        top = np.sort(l64, 1)
        gap = float((top[:, -1] - top[:, -2]).min())
        border = float(np.abs(cr.forward_offset_in_bias(st, crops, torch.float32) - l32).max())
        print(cc.case_id(case), "n", n, "softmax", dp, "logits", dl, "e32", e32, "smallest top-two gap", gap, "offset folded into the bias: logits move by", border)
        assert dp <= 1e-4 and dl <= 2e-3                            # the bars of test_cnn_arch_gpu.py
        assert np.array_equal(lab32, fx[pre + f"labels/{n}"]) and np.array_equal(lab64, lab32)
        assert e32 > 0 and gap >= 2 * cc.LOGIT_FACTOR * e32         # NO crop is undecided (the cap would allow UNDECIDED_CAP of them)
        assert border > 2e-3                                        # the padding clause bites: more than the logit bar


def test_negative_batchnorm_scales_reach_the_pool():
    for case in cc.CASES[:2]:
        st = cc.raw_state(case)
        for i, co in enumerate(weights.CATEGORY_CONVS, 1):
            g = st[f"batch_norm{i}.weight"]
            assert int((g < 0).sum()) == (co + 2) // 3 and g.shape == (co,)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("category_plan") / "print_category_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "print_category_plan.cpp"), "-o", path])
    return path


def plan(exe, w, h, ch):
    r = subprocess.run([exe, f"{w},{h},{ch}"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return dict(kv.split("=", 1) for kv in r.stdout.strip().split(" "))


def test_the_table_reaches_every_tile_width_with_ragged_edges(plan_exe):
    p = plan(plan_exe, 80, 80, 1)
    assert (p["name"], p["id"], p["n_conv"]) == ("category", "-1", "3")
    # 80 x 80: v100's plan with 3 taps; floats per crop 40*40*16 + 20*20*64 + 10*10*128 + 128 = 64128 -> 2^31 / 256513 = 8371.8
    assert p["L0"] == "1>16/16x1,t3,p2,80x80>40x40,16/3/9" and p["L1"] == "16>64/64x1,t3,p2,40x40>20x20,8/3/9"
    assert p["L2"] == "64>128/128x1,t3,p2,20x20>10x10,4/3/3" and (p["final"], p["K"], p["NH"], p["chunk"]) == ("10x10x128", "12800", "128", "8371")
    assert plan(plan_exe, 8, 8, 1)["chunk"] == str(1 << 16)         # ARCH_CHUNK_MAX: test_categorize_gpu.py's chunk boundary
    ragged, several = set(), set()
    for case in cc.CASES:
        w, h, ch, _ = case[0]
        p = plan(plan_exe, w, h, ch)
        for i in (1, 2):                                            # the convolutions of k_arch_conv
            geom, taps, pool, sizes, tiles = p[f"L{i}"].split(",")
            ho, wo = [int(v) for v in sizes.split(">")[1].split("x")]
            tx, tx_n, n_tiles = [int(v) for v in tiles.split("/")]
            ty = 64 // tx
            assert (taps, pool) == ("t3", "p2") and tx_n == -(-wo // tx) and n_tiles == tx_n * -(-ho // ty)
            if wo % tx and ho % ty:
                ragged.add(tx)
            if tx_n > 1 and n_tiles // tx_n > 1:
                several.add(tx)
    assert ragged == {4, 8, 16}                                     # all three tile widths at 3 taps with the pool, each ragged in x and in y
    assert several == {8}                                           # tile origins past 0 on both axes (80 x 80: 3 x 3 tiles in conv2); 4- and 16-wide tiles
                                                                    # stand several in a row (100 x 60: 7; 100 x 14: 2), never in a column: Ho < 16 there


def test_blob_round_trip_and_foreign_blobs():
    for (w, h, ch, cats) in ((8, 8, 1, 3), (21, 13, 3, 70)):
        st = weights.synthetic_category_state(cats, 4, ch, w, h)
        assert [n for n, _ in weights.category_shapes(cats, ch, w, h)][:8] == ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias",
                                                                                 "batch_norm1.weight", "batch_norm1.bias"]
        blob = weights.pack_category_blob(st, cats, ch, w, h)
        assert len(blob) == 32 + 4 * sum(int(np.prod(s)) for _, s in weights.category_shapes(cats, ch, w, h))
        assert np.frombuffer(blob[:32], np.int32).tolist() == [0x43585254, 1, cats, w, h, ch, 0, 0] and blob[:4] == b"TRXC"
        back, c2, ch2, w2, h2 = weights.unpack_category_blob(blob)
        assert (c2, ch2, w2, h2) == (cats, ch, w, h) and list(back) == list(st)
        assert all(back[k].tobytes() == st[k].tobytes() for k in st)
    with pytest.raises(AssertionError):
        weights.unpack_category_blob(weights.pack_blob(weights.synthetic_state(3, 1), 3))      # an identity blob
    with pytest.raises(AssertionError):
        weights.unpack_blob(blob)                                                               # ... and the reverse
    assert "category" not in weights.ARCH_IDS and len(weights.ARCH_IDS) == 5


def test_converter_round_trip_and_refusals():
    w, h, ch, cats = 21, 13, 3, 7
    st = weights.synthetic_category_state(cats, 8, ch, w, h)
    sd = {k: torch.from_numpy(v) for k, v in st.items()}
    sd["batch_norm1.num_batches_tracked"] = torch.tensor(3)
    blob, c2, ch2 = conv.convert({"model_state": sd, "samples": [], "labels": []}, w, h)
    assert (c2, ch2) == (cats, ch) and blob == weights.pack_category_blob(st, cats, ch, w, h)
    with pytest.raises(ValueError, match="model_state"):
        conv.convert(sd, w, h)                                      # a bare state_dict
    with pytest.raises(ValueError, match="model_state"):
        conv.convert({"state_dict": sd}, w, h)                      # an identity checkpoint
    with pytest.raises(ValueError, match="fc1.weight"):
        conv.convert({"model_state": sd}, 80, 80)                   # another size
    for name in ("conv2.bias", "batch_norm3.running_var", "fc2.bias"):
        with pytest.raises(ValueError, match=name):
            conv.convert({"model_state": {k: v for k, v in sd.items() if k != name}}, w, h)
    bad = dict(sd)
    bad["conv3.weight"] = torch.zeros(100, 64, 5, 5)
    with pytest.raises(ValueError, match="conv3.weight"):
        conv.convert({"model_state": bad}, w, h)
    with pytest.raises(ValueError, match="bn4.weight"):
        conv.convert({"model_state": dict(sd, **{"bn4.weight": torch.zeros(100)})}, w, h)


def test_vote_hand_cases():
    counts, rows, label, share, skipped = cr.vote([2, 0, 2, 0, -1, 5, 1], [1, 1, 1, 1, 1, 1, 3], 4, 3)
    assert counts.tolist() == [[0, 0, 0], [2, 0, 2], [0, 0, 0], [0, 1, 0]] and rows.tolist() == [0, 6, 0, 1]
    assert label.tolist() == [-1, 0, -1, 1]                         # a tie: the lowest index; an empty tracklet: -1
    assert skipped == 1 and not share[[0, 2]].any()                 # a label >= C: skipped and counted; shares of an empty tracklet: 0
    assert share[1].tolist() == [np.float32(2) / np.float32(6), 0.0, np.float32(2) / np.float32(6)] and share[3].tolist() == [0.0, 1.0, 0.0]
    assert share.dtype == np.float32 and counts.dtype == np.uint32  # the shares divide by ALL rows (6), not by the 4 valid ones
    counts, rows, label, share, skipped = cr.vote([-1, -1, -5], [0, 0, 0], 1, 2)
    assert label.tolist() == [-1] and rows.tolist() == [3] and skipped == 0 and not share.any()      # all rows unlabelled
    counts, rows, label, share, skipped = cr.vote([1, 0, 1, 0, 2, 2, 2], [0, 1, 0, 1, 0, 1, 1], 2, 3)
    assert counts.tolist() == [[0, 2, 1], [2, 0, 2]] and label.tolist() == [1, 0]                    # interleaved tracklets; tracklet 1 ties 0 and 2
    with pytest.raises(ValueError):
        cr.vote([0], [2], 2, 2)


def test_sample_rows_hand_cases():
    rows = lambda *a: cr.sample_rows(*a)[0].tolist()
    valid = lambda *a: cr.sample_rows(*a)[1]
    assert rows(1, 3, 50, 20) == [0] and not valid(1, 3, 50, 20)
    assert rows(14, 3, 50, 20) == list(range(14))                   # below 15: no offset; below min_samples: step 1
    assert rows(15, 3, 50, 20) == list(range(2, 15))                # 15 rows: offset 5 - 3 % 5 = 2
    assert rows(16, 10, 50, 20) == list(range(5, 16))               # a first frame divisible by 5: offset 5, not 0
    assert rows(16, 9, 50, 20) == list(range(1, 16))
    assert rows(19, 0, 50, 20) == list(range(5, 19)) and not valid(19, 0, 50, 20)       # min_samples - 1: step 1, 14 rows
    assert rows(20, 1, 50, 20) == list(range(4, 20)) and not valid(20, 1, 50, 20)       # min_samples: step max(1, 20 // 50) = 1, 16 rows after the offset
    assert rows(21, 4, 50, 20) == list(range(1, 21)) and valid(21, 4, 50, 20)           # min_samples + 1: 20 rows
    assert rows(300, 7, 50, 20) == list(range(3, 300, 6)) and valid(300, 7, 50, 20)     # step 300 // 50 = 6: 50 rows
    assert rows(40, 7, 3, 5) == [3, 16, 29] and not valid(40, 7, 3, 5)                  # step 13
