"""CPU side of the identity networks v100 / v110 / v119 / v200: the restatement tests/vi_arch_ref.py against the reference's own vectors
(tests/golden/cnn_arch.npz, made by tests/golden/make_cnn_arch_fixtures.py from the reference's modules) at the bars test_cnn_sizes_oracle.py
holds its oracle to -- 1e-5 on softmax, 2e-3 on logits in float32 --, the blob of every architecture both ways, and the converter."""
import importlib.util
import os
import numpy as np
import pytest
import torch
from trex_amd import weights
import vi_arch_ref
from vi_arch_ref import BATCHES, CASES, case_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("convert_weights", os.path.join(ROOT, "tools", "convert_weights.py"))
cw = importlib.util.module_from_spec(spec); spec.loader.exec_module(cw)
ALL = ("v118_3",) + vi_arch_ref.ARCHS


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_restatement_matches_the_reference_vectors(case):
    st, want, crops = vi_arch_ref.load_case(case)
    for n in BATCHES:
        probs, logits = want[n]
        p, lg = vi_arch_ref.forward(st, crops[n], case[0], torch.float32)
        assert p.shape == probs.shape == (n, case[4])
        print(case_id(case), n, "softmax", np.abs(p - probs).max(), "logits", np.abs(lg - logits).max())
        assert np.abs(p - probs).max() <= 1e-5, (n, np.abs(p - probs).max())
        assert np.abs(lg - logits).max() <= 2e-3, (n, np.abs(lg - logits).max())
    # the reference's own float32 error, against the same forward in float64: what the 1e-4 / 2e-3 bars of the device tests leave room for
    # (up to 2e-5 on softmax and 1e-4 on logits over these cases)
    p64, lg64 = vi_arch_ref.forward(st, crops[37], case[0], torch.float64)
    print(case_id(case), "float64 against the reference: softmax", np.abs(p64 - want[37][0]).max(), "logits", np.abs(lg64 - want[37][1]).max())
    assert np.abs(p64 - want[37][0]).max() <= 5e-5 and np.abs(lg64 - want[37][1]).max() <= 1e-3


def test_the_fixture_holds_what_its_generator_says():
    z = np.load(vi_arch_ref.GOLDEN)
    assert len(CASES) == 16
    for case in CASES:
        arch, w, h, ch, classes, seed = case
        pre = f"case/{case_id(case)}/"
        stats = [n for n, _ in weights.shapes(classes, ch, w, h, arch) if "running_" in n]
        assert sorted(k[len(pre) + 5:] for k in z.files if k.startswith(pre + "stat/")) == sorted(stats)
        for n in BATCHES:
            assert z[pre + f"probs/{n}"].shape == (n, classes) and z[pre + f"logits/{n}"].dtype == np.float32
    assert os.path.getsize(vi_arch_ref.GOLDEN) < (1 << 20)


def test_the_default_blob_is_what_it_always_was():
    st = weights.synthetic_state(8, 11)
    blob = weights.pack_blob(st, 8)
    hdr = np.array([weights.MAGIC, 1, 8, 80, 80, 1, 0, 0], np.int32).tobytes()
    assert blob == hdr + b"".join(np.ascontiguousarray(st[n], np.float32).tobytes() for n, _ in weights.TENSORS)
    assert blob == weights.pack_blob(st, 8, arch="v118_3") and weights.blob_arch(blob) == "v118_3"
    again = weights.synthetic_state(8, 11, arch="V118_3")
    assert list(again) == [n for n, _ in weights.TENSORS] and all(again[k].tobytes() == st[k].tobytes() for k in st)
    assert [n for n, _ in weights.shapes(8)] == [n for n, _ in weights.TENSORS]


@pytest.mark.parametrize("arch", ALL)
def test_blob_round_trip(arch):
    w, h, ch = 54, 30, 3
    st = weights.synthetic_state(5, 3, ch, w, h, arch=arch)
    assert list(st) == [n for n, _ in weights.shapes(5, ch, w, h, arch)]
    blob = weights.pack_blob(st, 5, ch, w, h, arch=arch)
    hdr = np.frombuffer(blob[:32], np.int32)
    assert list(hdr) == [weights.MAGIC, 1, 5, w, h, ch, weights.ARCH_IDS[arch], 0] and weights.blob_arch(blob) == arch
    assert len(blob) == 32 + 4 * sum(int(np.prod(s)) for _, s in weights.shapes(5, ch, w, h, arch))
    back, classes, channels = weights.unpack_blob(blob, arch)
    assert (classes, channels) == (5, ch) and list(back) == list(st)
    for k in st:
        assert back[k].tobytes() == st[k].tobytes(), k
    other = "v100" if arch != "v100" else "v110"
    with pytest.raises(AssertionError):
        weights.unpack_blob(blob, other)
    with pytest.raises(ValueError):
        weights.shapes(5, arch="v300")


def checkpoint(arch, classes, ch, w, h, label=None):
    st = weights.synthetic_state(classes, 7, ch, w, h, arch=arch)
    sd = {"model." + k: torch.from_numpy(v) for k, v in st.items()}
    for k in list(st):
        if k.endswith("running_var"):
            sd["model." + k.replace("running_var", "num_batches_tracked")] = torch.tensor(12345)
    return st, {"model": None, "state_dict": sd, "metadata": {"input_shape": (w, h, ch), "num_classes": classes, "model_type": label or arch}}


@pytest.mark.parametrize("arch", ALL)
def test_converter_both_ways(arch):
    st, ck = checkpoint(arch, 6, 1, 48, 32)
    blob, c, w, h, ch = cw.convert(ck)
    assert (c, w, h, ch) == (6, 48, 32, 1)
    assert blob == weights.pack_blob(st, 6, 1, 48, 32, arch=arch) and weights.blob_arch(blob) == arch
    back, _, _ = weights.unpack_blob(blob, arch)
    assert all(back[k].tobytes() == st[k].tobytes() for k in st)
    _, upper = checkpoint(arch, 6, 1, 48, 32, label=arch.upper())       # the reference's class names
    assert cw.convert(upper)[0] == blob


@pytest.mark.parametrize("arch", vi_arch_ref.ARCHS)
def test_converter_refuses_mislabelled_tensors(arch):
    for label in ALL:
        if label == arch:
            continue
        _, ck = checkpoint(arch, 6, 1, 48, 32, label=label)
        with pytest.raises(ValueError):
            cw.convert(ck)
    _, ck = checkpoint(arch, 6, 1, 48, 32)
    del ck["state_dict"]["model.fc2.bias"]
    with pytest.raises(ValueError):
        cw.convert(ck)
    _, ck = checkpoint(arch, 6, 1, 48, 32, label="convnext_base")
    with pytest.raises(ValueError):
        cw.convert(ck)
