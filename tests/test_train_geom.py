"""The geometry of the any-size training chain (trex_amd/csrc/train_geom.h) on the CPU: tests/cpp/test_train_geom.cpp prints it for each case, and
every expected number below is a literal worked out by hand from the rules the kernels are written to:
   levels        z1 = W x H, z2 = W/2 x H/2, z3 = (W/2)/2 x (H/2)/2, a3 = one more floor, P = a3's positions
   conv1         tiles of 16 x 16 pixels: ceil(W / 16) per row, times ceil(H / 16)
   conv2, conv3  tiles of 64 pool windows over ceil(h / 2) x ceil(w / 2) windows, shaped 8 x 8, 4 wide x 16 high or 16 wide x 4 high, whichever
                 gives the fewest (8 x 8 on a tie): printed as TX, tiles per row, tiles
   wgrad1        8 rows x 64 columns per workgroup: ceil(W / 64) per band, times ceil(H / 8)
   wgrad2/3      5 / 10 workgroup types; the n h rows of the batch in runs of per = ceil(rows / min(rows, 96 / 48)) rows: printed as types, per, shares
   bytes         4 x the element counts at a batch of 128; part = 4 x max(96 x 25 x 16 x 64, 48 x 25 x 64 x 128); part1 = 4 x n x tiles x CH x 400
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("train_geom") / ("test_train_geom_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_train_geom.cpp"), "-o", path])
    return path


def geom(exe, W, H, CH, n=128):
    r = subprocess.run([exe, f"{W},{H},{CH},{n}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return dict(kv.split("=", 1) for kv in r.stdout.strip().split(" "))


def has(g, **want):
    got = {k: g[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}, g


def test_the_smallest_size(exe):
    # 8 -> 4 -> 2 -> 1: conv3 sees 2 x 2 pixels = one window, one ragged tile everywhere; 128 x 4 = 512 rows in runs of ceil(512 / 96) = 6: 86 shares
    has(geom(exe, 8, 8, 1), z1="8x8", z2="4x4", z3="2x2", a3="1x1", P=1, conv1="1,1", conv2="8,1,1", conv3="8,1,1", wgrad1="1,1", wgrad2="5,6,86",
        wgrad3="10,6,43", x=32768, z="524288,524288,262144", a="131072,131072,65536", hpart=51200, part=39321600, part1=204800, f1w=51200)


def test_odd_levels_on_both_axes(exe):
    # 21 -> 10 -> 5 -> 2 and 13 -> 6 -> 3 -> 1: odd at levels 1 and 3; conv2's plane 10 x 6 = 5 x 3 windows, conv3's 5 x 3 = 3 x 2 windows (ceil)
    has(geom(exe, 21, 13, 3), z1="21x13", z2="10x6", z3="5x3", a3="2x1", P=2, conv1="2,2", conv2="8,1,1", conv3="8,1,1", wgrad1="1,2", wgrad2="5,8,96",
        wgrad3="10,8,48", x=419328, z="2236416,1966080,983040", a="491520,491520,131072", hpart=102400, part=39321600, part1=1228800, f1w=102400)
    # the transpose: the same counts with W and H swapped where they differ
    has(geom(exe, 13, 21, 1), z1="13x21", z2="6x10", z3="3x5", a3="1x2", P=2, conv1="1,2", conv2="8,1,1", conv3="8,1,1", wgrad1="1,3", wgrad2="5,14,92",
        wgrad3="10,14,46", x=139776, z="2236416,1966080,983040", a="491520,491520,131072", hpart=102400, part1=614400)


def test_several_tiles_with_a_ragged_last_one(exe):
    # conv2's plane 20 x 36 = 10 x 18 windows: 16 wide x 4 high tiles, 1 x 5 of them (8 x 8: 2 x 3 = 6); conv3's 10 x 18 = 5 x 9 windows: 8 x 8, 1 x 2
    has(geom(exe, 40, 72, 1), z1="40x72", z2="20x36", z3="10x18", a3="5x9", P=45, conv1="3,15", conv2="16,1,5", conv3="8,1,2", wgrad1="1,9", wgrad2="5,48,96",
        wgrad3="10,48,48", x=1474560, z="23592960,23592960,11796480", a="5898240,5898240,2949120", hpart=2304000, part1=1843200, f1w=2304000)
    # 100 x 60, three channels: conv2's plane 50 x 30 = 25 x 15 windows: 4 wide x 16 high, 7 x 1; a3 = 12 x 7 after three floors
    has(geom(exe, 100, 60, 3), z1="100x60", z2="50x30", z3="25x15", a3="12x7", P=84, conv1="7,28", conv2="4,7,7", conv3="8,2,2", wgrad1="2,16", wgrad2="5,40,96",
        wgrad3="10,40,48", x=9216000, z="49152000,49152000,24576000", a="12288000,12288000,5505024", hpart=4300800, part1=9830400, f1w=4300800)


def test_the_largest_size(exe):
    # 128 x 128 rows of conv2's plane at a batch of 128 = 16384 in runs of ceil(16384 / 96) = 171: 96 shares
    has(geom(exe, 256, 256, 1), z1="256x256", z2="128x128", z3="64x64", a3="32x32", P=1024, conv1="16,256", conv2="8,8,64", conv3="8,4,16", wgrad1="4,128",
        wgrad2="5,171,96", wgrad3="10,171,48", x=33554432, z="536870912,536870912,268435456", a="134217728,134217728,67108864", hpart=52428800,
        part=39321600, part1=26214400, f1w=52428800)


def test_the_shares_follow_the_batch(exe):
    # a last batch of an epoch: 7 crops of 21 x 13 are 42 rows of conv2's plane (one per share) and 21 of conv3's
    has(geom(exe, 21, 13, 1, n=7), wgrad2="5,1,42", wgrad3="10,1,21")
    has(geom(exe, 21, 13, 1, n=1), wgrad2="5,1,6", wgrad3="10,1,3")


def test_every_size_is_covered_exactly_once(exe):
    r = subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    assert r.stdout.strip() == "sweep ok 62001"          # 249 x 249 sizes
