"""The plan of the identity networks v100 / v110 / v119 / v200 (trex_amd/csrc/cnn_arch_plan.h) on the CPU: tests/cpp/test_cnn_arch_plan.cpp
prints the plan of each case, and every expected number below is a literal worked out by hand from the layer table of the issue:
   a layer's kernel writes Hi/2 x Wi/2 with its fused 2x2 pool, Hi x Wi without; k_pool3 behind it floors by 3
   tiles: 64 windows of 2x2 conv pixels, shaped 8x8, 4 wide x 16 high or 16 x 4 -- the fewest tiles, 8x8 on a tie; the first layer 16 x 16 windows
   channel blocks: 16 per workgroup in the first layer, else min(CO, 128); 100 channels are padded to 128
   chunk = floor(2 GiB / (4 * floats of every activation of one crop + 1)), at most 65536
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
V100, V110, V119, V200 = 1, 2, 3, 4


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_arch_plan") / ("test_cnn_arch_plan_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_arch_plan.cpp"), "-o", path])
    return path


def plan(exe, arch, W, H, CH=1):
    r = subprocess.run([exe, f"{arch},{W},{H},{CH}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return dict(kv.split("=", 1) for kv in r.stdout.strip().split(" "))


def has(p, **want):
    got = {k: p[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}, p


def test_v100_at_80x80(exe):
    # floats per crop: 40*40*16 + 20*20*64 + 10*10*128 + 128 = 64128 -> 256513 bytes; 2^31 / 256513 = 8371.8
    has(plan(exe, V100, 80, 80), name="v100", min=8, n_conv=3,
        L0="1>16/16x1,t5,p2,80x80>40x40>40x40,16/3/9", L1="16>64/64x1,t5,p2,40x40>20x20>20x20,8/3/9", L2="64>128/128x1,t5,p2,20x20>10x10>10x10,4/3/3",
        feat="10x10x128", K=12800, NH=128, planes=1, crop_bytes=256513, chunk=8371)


def test_v110_colour_non_square(exe):
    # W = 100, H = 60: 60x100 -> 30x50 -> 15x25 -> 7x12; 15 x 25 windows: 8x8 8 tiles, 4 wide x 16 high 7, 16 x 4 8
    has(plan(exe, V110, 100, 60, 3), name="v110", L0="3>16/16x1,t5,p2,60x100>30x50>30x50,16/4/8", L1="16>64/64x1,t5,p2,30x50>15x25>15x25,4/7/7",
        L2="64>128/128x1,t5,p2,15x25>7x12>7x12,8/2/2", feat="7x12x128", K=10752, NH=128)


def test_v119_at_its_minimum(exe):
    # 16*16/4*256 + 4*4*128 + 2*2*32 + 128 + 1024 = 19712 floats -> 78849 bytes; 2^31 / 78849 = 27235.3
    has(plan(exe, V119, 16, 16), name="v119", min=16, n_conv=4, L0="1>256/16x16,t5,p2,16x16>8x8>8x8,16/1/1", L1="256>128/128x1,t5,p2,8x8>4x4>4x4,8/1/1",
        L2="128>32/32x1,t5,p2,4x4>2x2>2x2,8/1/1", L3="32>128/128x1,t5,p2,2x2>1x1>1x1,8/1/1", feat="1x1x128", K=128, NH=1024, planes=1, crop_bytes=78849,
        chunk=27235)


def test_v200_at_80x80(exe):
    # 80 -> 26 -> 8 -> 2; floats 409600 + 819200 + 86528 + 173056 + 346112 + 32768 + 32768 + 2048 + 512 + 1024 = 1903616 -> 7614465 bytes
    has(plan(exe, V200, 80, 80), name="v200", min=27, n_conv=5, L0="1>64/16x4,t3,p0,80x80>80x80>80x80,16/3/9", L1="64>128/128x1,t3,p3,80x80>80x80>26x26,8/5/25",
        L2="128>256/128x2,t3,p0,26x26>26x26>26x26,8/2/4", L3="256>512/128x4,t3,p3,26x26>26x26>8x8,8/2/4", L4="512>512/128x4,t3,p3,8x8>8x8>2x2,8/1/1",
        feat="2x2x512", K=512, NH=1024, planes=1, crop_bytes=7614465, chunk=282)


def test_chunks_at_the_extremes(exe):
    # v200 at 256x256: 19902336 floats -> 79609345 bytes -> 26 crops; v100 at 8x8: 768 floats -> far more than 65536 fit
    has(plan(exe, V200, 256, 256), crop_bytes=79609345, chunk=26, feat="9x9x512")
    has(plan(exe, V100, 8, 8), crop_bytes=4 * (4 * 4 * 16 + 2 * 2 * 64 + 128 + 128) + 1, chunk=65536, K=128)
    has(plan(exe, V200, 27, 27), feat="1x1x512", L4="512>512/128x4,t3,p3,3x3>3x3>1x1,8/1/1")


def test_the_chunk_does_not_depend_on_the_channels_of_the_crop(exe):
    # the crop itself is not an activation: 1 and 3 channels have the same plan behind the first layer's CI
    a, b = plan(exe, V119, 80, 80, 1), plan(exe, V119, 80, 80, 3)
    assert a["chunk"] == b["chunk"] and a["L1"] == b["L1"] and a["L0"].replace("1>256", "3>256") == b["L0"]
