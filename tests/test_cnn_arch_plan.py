"""The plan of the identity networks v100 / v110 / v119 / v200 (trex_amd/csrc/cnn_arch_plan.h) on the CPU: tests/cpp/test_cnn_arch_plan.cpp
prints the plan of each case, and every expected number below is a literal worked out by hand from the layer table of the issue:
   a layer's kernel writes Hi/2 x Wi/2 with its fused 2x2 pool, Hi x Wi without; k_pool3 behind it floors by 3
   tiles: 64 windows of 2x2 conv pixels, shaped 8x8, 4 wide x 16 high or 16 x 4 -- the fewest tiles, 8x8 on a tie; the first layer 16 x 16 windows
   channel blocks: 16 per workgroup in the first layer, else min(CO, 128); 100 channels are padded to 128
   chunk = floor(2 GiB / (4 * floats of every activation of one crop + 1)), at most 65536
The second half holds the edge-case table (cnn_arch_edge_cases.py) to what it claims to reach, again against a hand-made list.
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


# ---- what the edge-case table (cnn_arch_edge_cases.py) reaches: the proof, without a GPU, of what test_cnn_arch_edges_gpu.py runs ----
# Every (taps, pool inside the kernel, channels per workgroup) a layer behind the first can have, from the layer table:
#   v100 / v110: conv2 16 -> 64 and conv3 64 -> 100 (padded to 128), 5 taps, fused 2x2 pool              (5, 2, 64)  (5, 2, 128)
#   v119: conv2 256 -> 128, conv3 128 -> 32, conv4 32 -> 128, 5 taps, fused 2x2 pool                      (5, 2, 128) (5, 2, 32)
#   v200: conv2 .. conv5 to 128, 256, 512, 512 in blocks of 128, 3 taps, no pool in the kernel (pool 3 is k_pool3's)   (3, 0, 128)
# and each of them under each of the three tile shapes, which depend on the layer's size alone: 4 x 3 = 12 combinations.
REACHABLE = [(tx, taps, pool, cob) for tx in (4, 8, 16) for taps, pool, cob in ((5, 2, 32), (5, 2, 64), (5, 2, 128), (3, 0, 128))]
# the first layer (k_arch_conv1<CH, T>): v100 / v110 / v119 5 taps with the pool, v200 3 taps without, each with 1 and 3 channels
FIRST = [(5, 2, 1), (5, 2, 3), (3, 0, 1), (3, 0, 3)]


def _layer(text):
    """'16>64/64x1,t5,p2,6x34>3x17>3x17,16/2/2' -> dict of its numbers"""
    io, t, p, sizes, tl = text.split(",")
    ci, rest = io.split(">")
    co, blk = rest.split("/")
    cob, blocks = blk.split("x")
    (hi, wi), (ho, wo), (h3, w3) = [tuple(int(v) for v in s.split("x")) for s in sizes.split(">")]
    tx, tx_n, tiles = [int(v) for v in tl.split("/")]
    return dict(CI=int(ci), CO=int(co), COB=int(cob), blocks=int(blocks), taps=int(t[1:]), pool=int(p[1:]), Hi=hi, Wi=wi, Ho=ho, Wo=wo, H3=h3, W3=w3,
                TX=tx, tx_n=tx_n, tiles=tiles)


def test_the_edge_table_reaches_every_tile_shape_with_ragged_edges(exe):
    from cnn_arch_edge_cases import CASES, MIN_LOGITS, case_id
    from trex_amd import weights
    ragged = {c: set() for c in REACHABLE}                   # combination -> {"x", "y"}
    first = {c: set() for c in FIRST}                        # first-layer instance -> {"odd W", "odd H"}
    blocks16, left = set(), {False: set(), True: set()}     # channel blocks under the 16-wide tile; gap? -> positions the last layer leaves
    for case in CASES:
        arch, W, H, CH, classes, n, _, _ = case
        assert n * classes >= MIN_LOGITS, case_id(case)
        p = plan(exe, weights.ARCH_IDS[arch], W, H, CH)
        assert W >= int(p["min"]) and H >= int(p["min"]) and W <= 256 and H <= 256 and int(p["chunk"]) >= n, case_id(case)
        L = [_layer(p[f"L{i}"]) for i in range(int(p["n_conv"]))]
        l0 = L[0]
        assert (l0["Hi"], l0["Wi"], l0["CI"]) == (H, W, CH)
        kind = (l0["taps"], l0["pool"], CH)
        assert kind in first, (case_id(case), kind)
        first[kind] |= ({"odd W"} if W % 2 else set()) | ({"odd H"} if H % 2 else set())
        for l in L[1:]:
            fused = l["pool"] == 2
            wy, wx = (l["Ho"], l["Wo"]) if fused else ((l["Hi"] + 1) // 2, (l["Wi"] + 1) // 2)          # windows of 2 x 2 conv pixels
            tx, ty = l["TX"], 64 // l["TX"]
            assert l["tx_n"] == -(-wx // tx) and l["tiles"] == l["tx_n"] * -(-wy // ty), (case_id(case), l)
            combo = (tx, l["taps"], 2 if fused else 0, l["COB"])
            assert combo in ragged, (case_id(case), combo)           # nothing outside the hand-made list
            ragged[combo] |= ({"x"} if wx % tx else set()) | ({"y"} if wy % ty else set())
            if tx == 16:
                blocks16.add(l["blocks"])
        hf, wf, _ = [int(v) for v in p["feat"].split("x")]
        left[arch == "v200"].add(hf * wf)
    assert all(v == {"x", "y"} for v in ragged.values()), {k: v for k, v in ragged.items() if v != {"x", "y"}}
    assert all(v == {"odd W", "odd H"} for v in first.values()), first
    assert blocks16 == {1, 2, 4}                                                                         # v200: 128, 256 and 512 output channels
    assert all(1 in v and max(v) > 1 for v in left.values()), left                                      # 1x1 and more than one position: flatten and average
    assert {c[4] for c in CASES} >= {1, 2, 63, 64, 65, 100, 257, 1024}                                   # the head's repetitions
    assert {c[5] for c in CASES} >= {1, 31, 32, 33} and max(c[5] for c in CASES) > 64                    # fc1's row blocks, the head's 4 crops per workgroup


def test_plans_of_the_16_wide_cases(exe):
    # v100 at W = 69, H = 13: 13x69 -> 6x34 -> 3x17 -> 1x8.  3 x 17 windows: 8x8 3 tiles, 4 wide x 16 high 5, 16 x 4 2
    has(plan(exe, V100, 69, 13), L0="1>16/16x1,t5,p2,13x69>6x34>6x34,16/3/3", L1="16>64/64x1,t5,p2,6x34>3x17>3x17,16/2/2",
        L2="64>128/128x1,t5,p2,3x17>1x8>1x8,8/1/1", feat="1x8x128", K=1024)
    # v119 at 75x19: 19x75 -> 9x37 -> 4x18 -> 2x9 -> 1x4.  4 x 18: 8x8 3, 4 wide 5, 16 wide 2; 2 x 9: 8x8 2, 4 wide 3, 16 wide 1
    has(plan(exe, V119, 75, 19), L1="256>128/128x1,t5,p2,9x37>4x18>4x18,16/2/2", L2="128>32/32x1,t5,p2,4x18>2x9>2x9,16/1/1",
        L3="32>128/128x1,t5,p2,2x9>1x4>1x4,8/1/1", feat="1x4x128")
    # v119 at 137x27: 27x137 -> 13x68 -> 6x34 -> 3x17 -> 1x8.  6 x 34: 8x8 5, 4 wide 9, 16 wide 6; 3 x 17 as above
    has(plan(exe, V119, 137, 27), L1="256>128/128x1,t5,p2,13x68>6x34>6x34,8/5/5", L2="128>32/32x1,t5,p2,6x34>3x17>3x17,16/2/2")
    # v200 at 93x54: 54x93 -> (pool 3) 18x31 -> 6x10 -> 2x3.  27 x 47 windows: 8x8 4 * 6 = 24, 4 wide 2 * 12 = 24, 16 wide 7 * 3 = 21;
    # 9 x 16: 8x8 4, 4 wide 4, 16 wide 3; 3 x 5: one tile of each, 8x8 on the tie
    has(plan(exe, V200, 93, 54), L1="64>128/128x1,t3,p3,54x93>54x93>18x31,16/3/21", L2="128>256/128x2,t3,p0,18x31>18x31>18x31,16/1/3",
        L3="256>512/128x4,t3,p3,18x31>18x31>6x10,16/1/3", L4="512>512/128x4,t3,p3,6x10>6x10>2x3,8/1/1", feat="2x3x512", K=512)
    # ... and its transpose takes the 4-wide tile
    has(plan(exe, V200, 54, 93), L1="64>128/128x1,t3,p3,93x54>93x54>31x18,4/7/21", L2="128>256/128x2,t3,p0,31x18>31x18>31x18,4/3/3", feat="3x2x512")


def test_the_chunk_does_not_depend_on_the_channels_of_the_crop(exe):
    # the crop itself is not an activation: 1 and 3 channels have the same plan behind the first layer's CI
    a, b = plan(exe, V119, 80, 80, 1), plan(exe, V119, 80, 80, 3)
    assert a["chunk"] == b["chunk"] and a["L1"] == b["L1"] and a["L0"].replace("1>256", "3>256") == b["L0"]
