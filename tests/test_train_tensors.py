"""The tensor table of the trainers (trex_amd/csrc/train_tensors.h) on the CPU: tests/cpp/print_train_tensors.cpp prints it for the four networks
that train (V118_3, v100, v110, the category network) at 8x8x1, 21x13x3 and 80x80x1, and this file holds every line to
   the shapes of trex_amd/weights.py   the torch counts in the state_dict order equal shapes(..., arch=...) / category_shapes, element count by
                 element count and in the same order; Adam's skip list names exactly the slots of the running_mean / running_var entries
   arithmetic    to_internal puts every element of every tensor inside [0, isz) and no two of a tensor in one place (the program walks all of
                 them); every offset is a multiple of 64 floats, the ranges [off, off + isz) do not overlap and end inside `total`
   literals      the bytes of one sample's dropout masks, worked out by hand:
                 V118_3       16 + 64 + 128 channels (Dropout2d behind each block) + 100 (Dropout behind fc1)              = 308 at every size
                 v100, v110   16 + 64 + 100 + 100                                                                          = 280 at every size
                 category     one byte per pooled element of the real channels (nn.Dropout), the planes by successive floors:
                              8 x 8      4x4x16 + 2x2x64 + 1x1x100 + 100     = 256 + 256 + 100 + 100                       = 712
                              21 x 13    10x6x16 + 5x3x64 + 2x1x100 + 100    = 960 + 960 + 200 + 100                       = 2220
                              80 x 80    40x40x16 + 20x20x64 + 10x10x100 + 100 = 25600 + 25600 + 10000 + 100               = 61300
                 and the planes' offsets are the running sums of those terms
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import numpy as np
import pytest
from trex_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NETS = ["v118_3", "v100", "v110", "category"]
SIZES = [(8, 8, 1), (21, 13, 3), (80, 80, 1)]
CLASSES = 7
KEEP = {"v118_3": (16, 64, 128, 100), "v100": (16, 64, 100, 100), "v110": (16, 64, 100, 100),
        ("category", 8, 8): (256, 256, 100, 100), ("category", 21, 13): (960, 960, 200, 100), ("category", 80, 80): (25600, 25600, 10000, 100)}
KEEP_ROW = {"v118_3": 308, "v100": 280, "v110": 280, ("category", 8, 8): 712, ("category", 21, 13): 2220, ("category", 80, 80): 61300}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("train_tensors") / ("print_train_tensors_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "print_train_tensors.cpp"), "-o", path])
    return path


@pytest.fixture(scope="module")
def tables(exe):
    """{(net, W, H, CH): the printed line as a dict, lists as lists of int}: one run of the program for all twelve"""
    cases = [(net, W, H, CH) for net in NETS for W, H, CH in SIZES]
    r = subprocess.run([exe] + [f"{NETS.index(net)},{W},{H},{CH},{CLASSES}" for net, W, H, CH in cases], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    out = {}
    for case, line in zip(cases, lines):
        d = dict(kv.split("=", 1) for kv in line.split(" "))
        out[case] = {k: [int(x) for x in v.split(",") if x] if k in ("order", "cnt", "isz", "off", "keep_off", "buffers") else int(v) for k, v in d.items()}
    return out


def shapes(net, W, H, CH):
    return weights.category_shapes(CLASSES, CH, W, H) if net == "category" else weights.shapes(CLASSES, CH, W, H, arch=net)


@pytest.mark.parametrize("net", NETS)
def test_torch_counts_and_order(tables, net):
    for W, H, CH in SIZES:
        t = tables[(net, W, H, CH)]
        assert t["cnt"] == [int(np.prod(shp)) for _, shp in shapes(net, W, H, CH)], (net, W, H, CH)
        assert t["taps"] == (3 if net == "category" else 5)
        assert len(set(t["order"])) == len(t["order"]) and max(t["order"]) < t["slots"]
        if net == "v118_3":
            assert t["order"] == list(range(24)) and t["isz"] == t["cnt"]          # the blob's tensor ids, nothing padded


@pytest.mark.parametrize("net", NETS)
def test_to_internal_is_injective_and_inside(tables, net):
    for W, H, CH in SIZES:
        t = tables[(net, W, H, CH)]
        assert t["outside"] == 0 and t["twice"] == 0, (net, W, H, CH)
        assert all(i >= c for i, c in zip(t["isz"], t["cnt"]))


@pytest.mark.parametrize("net", NETS)
def test_offsets(tables, net):
    for W, H, CH in SIZES:
        t = tables[(net, W, H, CH)]
        assert all(o % 64 == 0 for o in t["off"]) and t["total"] % 64 == 0
        spans = sorted(zip(t["off"], t["isz"]))
        assert all(o + n <= o2 for (o, n), (o2, _) in zip(spans, spans[1:])), (net, W, H, CH)
        assert spans[-1][0] + spans[-1][1] <= t["total"]
        assert t["total"] == sum((n + 63) // 64 * 64 for n in t["isz"])              # nothing but the tensors and their padding


@pytest.mark.parametrize("net", NETS)
def test_mask_planes(tables, net):
    for W, H, CH in SIZES:
        t = tables[(net, W, H, CH)]
        key = (net, W, H) if net == "category" else net
        assert t["keep_row"] == KEEP_ROW[key], (net, W, H)
        assert t["keep_off"] == [int(x) for x in np.cumsum((0,) + KEEP[key][:3])], (net, W, H)


@pytest.mark.parametrize("net", NETS)
def test_adam_skips_exactly_the_running_statistics(tables, net):
    for W, H, CH in SIZES:
        t = tables[(net, W, H, CH)]
        want = [t["order"][i] for i, (name, _) in enumerate(shapes(net, W, H, CH)) if name.endswith(("running_mean", "running_var"))]
        assert sorted(t["buffers"]) == sorted(want), (net, W, H, CH)
        assert len(want) == {"v118_3": 6, "v100": 0, "v110": 8, "category": 6}[net]
