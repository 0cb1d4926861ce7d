"""The windowed listed conv3's rule in x, its windows and the packing of its passes (trex_amd/csrc/cnn_skip3.h) on the CPU:
tests/cpp/test_cnn_skip3x.cpp prints what the header says, and this file propagates the dependence by brute force on sets of columns and rows,
without the header's formulas:
   5 x 5 'same' convolution: output column x reads input columns x - 2 .. x + 2 that exist;  2 x 2 max-pool: output column c reads 2 c, 2 c + 1
   crop (80) -> conv -> pool (40, V2) -> conv -> pool (20, V3) -> conv3 (20 columns); an F(4,5) tile is 4 of those: 5 tiles, each reading an
   8-column window of V3; a row pair is two of conv3's rows
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NONE = (80, -1)
WT3, SLOTS, NR, ROWB, TILEB = 3, 10, 28, 10240, 32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_skip3x") / ("test_cnn_skip3x_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_skip3x.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


def conv(dirty, size):
    return {x for x in range(size) if any(0 <= x + k < size and x + k in dirty for k in (-2, -1, 0, 1, 2))}


def pool(dirty, size):
    return {c for c in range(size // 2) if 2 * c in dirty or 2 * c + 1 in dirty}


def v3_of(a, b):
    """the V3 columns (or rows) that differ from the empty crop's, for non-zero crop columns (rows) a .. b"""
    return pool(conv(pool(conv(set(range(a, b + 1)), 80), 80), 40), 40)


def tiles_of(x0, x1):
    """conv3's tiles of a crop whose non-zero columns lie in x0 .. x1, two ways: through conv3's output columns, and through the 8-column window
    of V3 that each tile reads"""
    v3 = v3_of(x0, x1)
    out = conv(v3, 20)
    by_output = {t for t in range(5) if any(4 * t + k in out for k in range(4))}
    by_window = {t for t in range(5) if any(c in v3 for c in range(4 * t - 2, 4 * t + 6))}
    assert by_output == by_window
    return by_window


def pairs_of(y0, y1):
    out = conv(v3_of(y0, y1), 20)
    return {q for q in range(10) if 2 * q in out or 2 * q + 1 in out}


def test_tile_range_of_every_column_band(exe):
    lines = run(exe, "tiles")
    assert len(lines) == 1 + 80 * 81 // 2 == 3241
    seen = set()
    for line in lines:
        x0, x1, lo, hi = map(int, line.split())
        seen.add((x0, x1))
        want = tiles_of(x0, x1) if x0 <= x1 else set()
        assert set(range(lo, hi + 1)) == want, (x0, x1, lo, hi, sorted(want))
        assert want == set(range(min(want), max(want) + 1)) if want else lo > hi
    assert NONE in seen and all((a, b) in seen for a in range(80) for b in range(a, 80))
    # the numbers of the rule, by hand: tile t reads crop columns 16 t - 14 .. 16 t + 29
    assert tiles_of(0, 0) == {0} and tiles_of(2, 2) == {0, 1} and tiles_of(18, 18) == {0, 1, 2} and tiles_of(29, 29) == {0, 1, 2} and tiles_of(30, 30) == {1, 2}
    assert tiles_of(79, 79) == {4} and tiles_of(77, 77) == {3, 4} and tiles_of(34, 45) == {1, 2, 3}


def window(exe, x0, x1, out_of_range=0):
    return int(run(exe, "window", x0, x1, out_of_range)[0])


def test_windows(exe):
    # exactly WT3 tiles at t0 = 0, 1, 2
    assert tiles_of(0, 33) == {0, 1, 2} and window(exe, 0, 33) == 0
    assert tiles_of(30, 49) == {1, 2, 3} and window(exe, 30, 49) == 1
    assert tiles_of(46, 79) == {2, 3, 4} and window(exe, 46, 79) == 2
    # one column more in either direction: four tiles, no window
    assert tiles_of(0, 34) == {0, 1, 2, 3} and window(exe, 0, 34) == -1
    assert tiles_of(29, 49) == {0, 1, 2, 3} and window(exe, 29, 49) == -1
    assert tiles_of(30, 50) == {1, 2, 3, 4} and window(exe, 30, 50) == -1
    assert tiles_of(45, 79) == {1, 2, 3, 4} and window(exe, 45, 79) == -1
    assert window(exe, 0, 79) == -1
    # fewer than WT3 tiles at the right edge: the window is moved left so that it ends at tile 4
    assert tiles_of(79, 79) == {4} and window(exe, 79, 79) == 2 and window(exe, 0, 0) == 0
    # no column band: no pair to compute and no window; the empty crop's image not to be used: no window, however narrow the blob
    assert window(exe, *NONE) == -1 and window(exe, 40, 40, 1) == -1 and window(exe, *NONE, 1) == -1
    # every band: a window holds every tile of the band, lies inside the row, is as far left as that allows, and is refused only above WT3 tiles
    lines = run(exe, "windows")
    assert len(lines) == 80 * 81 // 2
    for line in lines:
        x0, x1, w = map(int, line.split())
        t = tiles_of(x0, x1)
        if len(t) > WT3:
            assert w == -1, (x0, x1)
        else:
            assert w == min(min(t), 5 - WT3) and max(t) < w + WT3, (x0, x1, w)


def packed(exe, total, first, crops):
    passes = []
    for line in run(exe, "pack", total, first, *("%d:%d:%d:%d" % (b + c) for b, c in crops)):
        f = line.split()
        if f[0] == "pass":
            passes.append({"pairs": int(f[2]), "runs": int(f[3]), "rows": int(f[4]), "base": int(f[5]), "slots": [], "src": {}})
        elif f[0] == "slot":
            passes[-1]["slots"].append(tuple(map(int, f[2:])))
        else:
            passes[-1]["src"][int(f[1])] = (int(f[2]), int(f[3]))
    return passes


def check_block(exe, total, first, crops):
    """every listed pair of every windowed crop in exactly one slot; a pass within its slots, runs and rows; every LDS row a slot's pair reads
    comes from byte t0 * 32 of the right row: V3 (behind the front image's 20 rows) where the crop's own rows are, else either image"""
    passes = packed(exe, total, first, crops)
    want = {}
    for k, ((y0, y1), (x0, x1)) in enumerate(crops):
        t = tiles_of(x0, x1) if x0 <= x1 else set()
        if y0 <= y1 and 0 < len(t) <= WT3:
            for q in pairs_of(y0, y1):
                want[(first + k) * 10 + q] = (q, min(min(t), 5 - WT3))
    seen = []
    for p in passes:
        live = [s for s in p["slots"] if s[0] >= 0]
        assert len(p["slots"]) == SLOTS and len(live) == p["pairs"] <= SLOTS and p["runs"] <= 2 and p["rows"] <= NR
        assert [s[0] for s in live] == sorted(s[0] for s in live) and p["slots"][:len(live)] == live
        assert sum(1 for a, b in zip(live, live[1:]) if b[0] != a[0] + 1 or b[0] // 10 != a[0] // 10) + 1 <= p["runs"]
        used = set()
        for gp, q, t0, lds in live:
            seen.append(gp)
            assert want[gp] == (q, t0), (gp, q, t0)
            crop = gp // 10
            (y0, y1), _ = crops[crop - first]
            own = v3_of(y0, y1)
            for k in range(-2, 4):
                y, i = 2 * q + k, lds - 1 + k
                if not 0 <= y < 20:
                    continue
                assert 0 <= i < p["rows"], (gp, k, i)
                row, byte = p["src"][i]
                used.add(i)
                assert byte == t0 * TILEB, (gp, k, byte)
                assert row == (20 + crop * 20 + y if y in own else row if row in (y, 20 + 20 * total + y) else -2), (gp, k, row)
                assert 0 <= (row - p["base"]) * ROWB < 0xF0000000
        assert used == set(range(p["rows"]))                                        # no row staged for nothing
        assert all(p["src"][i] == (-1, -1) for i in range(p["rows"], 31))
    assert sorted(seen) == sorted(want)
    return passes


def test_packing_of_windowed_runs(exe):
    narrow, wide = (40, 41), (0, 79)
    # ten pairs of one crop fill a pass: one run, 20 rows (no halo outside the crop)
    (p,) = check_block(exe, 4, 2, [((0, 79), narrow)])
    assert (p["pairs"], p["runs"], p["rows"]) == (10, 1, 20)
    # two runs must split by rows: 7 + 7 pairs -> 7 + 3 (28 rows with the halos inside the crops), then 4
    a, b = check_block(exe, 9, 0, [((30, 57), narrow), ((30, 57), (0, 1))])
    assert (a["pairs"], a["runs"], b["pairs"], b["runs"]) == (10, 2, 4, 1) and a["rows"] <= NR
    # a crop without a window between two with one is not in this list; an empty crop has no run
    ps = check_block(exe, 9, 3, [((10, 20), narrow), ((10, 20), wide), (NONE, NONE), ((60, 79), (78, 79))])
    assert len(ps) == 1 and ps[0]["runs"] == 2
    # a third run closes a pass: single pixels
    ps = check_block(exe, 40, 0, [((r, r), ((37 * r + 11) % 80,) * 2) for r in range(0, 80, 3)][:32])
    assert len(ps) == 14 and all(p["runs"] == 2 for p in ps[:13])
    # a batch whose far end only the image behind V3 serves (25600 crops: 5.2 GB of V3)
    check_block(exe, 25600, 25568, [((8 * (k % 9), 8 * (k % 9) + 12), (5 * k % 70, 5 * k % 70 + 9)) for k in range(32)])
    check_block(exe, 25600, 0, [((8 * (k % 9), 8 * (k % 9) + 12), (5 * k % 70, 5 * k % 70 + 9)) for k in range(32)])
    # every row band at t0 = 1, beside a tall neighbour
    for y0 in range(0, 80, 7):
        for y1 in range(y0, 80, 5):
            check_block(exe, 3, 0, [((y0, y1), narrow), ((0, 79), (70, 79))])


def test_the_switch_is_bit_21_of_the_geometry_word(exe):
    assert run(exe, "plan", 0, 3200) == ["skip3=1 v3_direct=1 skip3x=1"]
    assert run(exe, "plan", 1 << 21, 3200) == ["skip3=1 v3_direct=1 skip3x=0"]
    assert run(exe, "plan", 1 << 25, 3200) == ["skip3=1 v3_direct=0 skip3x=0"]          # the listed form reads a copy: no windows
    assert run(exe, "plan", 1 << 26, 3200) == ["skip3=0 v3_direct=0 skip3x=0"]
    assert run(exe, "plan", 1 << 29, 1) == ["skip3=1 v3_direct=1 skip3x=1"]
    assert run(exe, "plan", 0, 40000) == ["skip3=1 v3_direct=0 skip3x=0"]               # 8 GB of V3: out of both images' reach
    for geom, n in ((0, 3199), (1 << 30, 12800), (1 << 28, 12800), (1, 12800), (1 << 27, 12800)):
        assert run(exe, "plan", geom, n)[0].endswith("skip3x=0")
