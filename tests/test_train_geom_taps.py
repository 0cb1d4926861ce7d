"""The tap count in the geometry of the any-size training chain (trex_amd/csrc/train_geom.h) on the CPU: tests/cpp/test_train_geom_taps.cpp prints it,
and every expected number below is a literal worked out by hand:
   wgrad2/3      a workgroup type is a kernel row x a 32-wide slice of the input channels: taps types for conv2 (16 channels: one slice), 2 taps for
                 conv3 (64 channels: two) -- 3 and 6 at 3 taps, 5 and 10 at 5; the shares do not depend on the tap count
   part          4 x max(96 x taps^2 x 16 x 64, 48 x taps^2 x 64 x 128) bytes: 4 x 9 x 393216 = 14155776 at 3 taps, 4 x 25 x 393216 = 39321600 at 5
   part1         4 x n x strips x CH x taps^2 x 16 bytes
   everything else -- levels, tiles, strips, activation sizes, fc1 -- is the tap count's business nowhere
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("train_geom_taps") / ("test_train_geom_taps_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_train_geom_taps.cpp"), "-o", path])
    return path


def geom(exe, W, H, CH, n, taps):
    r = subprocess.run([exe, f"{W},{H},{CH},{n},{taps}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return dict(kv.split("=", 1) for kv in r.stdout.strip().split(" "))


def has(g, **want):
    got = {k: g[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}, g


def test_three_taps(exe):
    # 21 x 13 x 3 at n = 128: 128 x 6 = 768 rows of conv2's plane in runs of 8: 96 shares; 384 of conv3's in 48; two 8-row bands of one 64-column strip
    has(geom(exe, 21, 13, 3, 128, 3), taps=3, z3="5x3", P=2, conv2="8,1,1", conv3="8,1,1", wgrad1="1,2", wgrad2="3,8,96", wgrad3="6,8,48", part=14155776,
        part1=4 * 128 * 2 * 3 * 144, z=983040, a=131072, f1w=102400)
    # 100 x 60 x 1 at n = 3: 90 rows and 45 rows, one per share; 2 strips x 8 bands
    has(geom(exe, 100, 60, 1, 3, 3), taps=3, conv2="4,7,7", conv3="8,2,2", wgrad1="2,16", wgrad2="3,1,90", wgrad3="6,1,45", part=14155776, part1=4 * 3 * 16 * 144)


def test_the_default_is_five_taps_and_unchanged(exe):
    want = dict(taps=5, z3="5x3", P=2, conv2="8,1,1", conv3="8,1,1", wgrad1="1,2", wgrad2="5,8,96", wgrad3="10,8,48", part=39321600, part1=1228800, z=983040,
                a=131072, f1w=102400)                            # test_train_geom.py's numbers at 21 x 13 x 3
    has(geom(exe, 21, 13, 3, 128, 0), **want)
    has(geom(exe, 21, 13, 3, 128, 5), **want)
    has(geom(exe, 256, 256, 1, 128, 0), wgrad2="5,171,96", wgrad3="10,171,48", part=39321600, part1=26214400)
