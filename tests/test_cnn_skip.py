"""Which rows of conv2's pooled output depend on which crop rows (trex_amd/csrc/cnn_skip.h) on the CPU: tests/cpp/test_cnn_skip.cpp prints what the
rule says, and this file propagates the dependence by brute force, layer by layer on sets of rows, without the rule's formulas:
   5 x 5 'same' convolution: output row y reads input rows y - 2 .. y + 2 that exist;  2 x 2 max-pool: output row r reads rows 2 r, 2 r + 1
   crop (80 rows) -> conv -> pool (40) -> conv -> pool (20 rows per crop = the V3 rows; a pass of the kernel is 3 consecutive V3 rows of the batch)
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import random
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NONE = (80, -1)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_skip") / ("test_cnn_skip_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_skip.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


def conv_rows(dirty, rows):
    """rows of a 5 x 5 'same' convolution's output that read a dirty input row"""
    return {y for y in range(rows) if any(0 <= y + k < rows and y + k in dirty for k in (-2, -1, 0, 1, 2))}


def pool_rows(dirty, rows):
    return {r for r in range(rows // 2) if 2 * r in dirty or 2 * r + 1 in dirty}


def v3_rows(y0, y1):
    """the V3 rows of a crop whose non-zero rows lie in y0 .. y1 (every one of them taken as non-zero: the rule knows no more)"""
    d = set(range(y0, y1 + 1))
    d = pool_rows(conv_rows(d, 80), 80)
    d = pool_rows(conv_rows(d, 40), 40)
    return d


_brute = {}


def brute(y0, y1):
    if (y0, y1) not in _brute:
        _brute[(y0, y1)] = v3_rows(y0, y1)
    return _brute[(y0, y1)]


def test_row_range_of_every_band(exe):
    lines = run(exe, "rows")
    assert len(lines) == 1 + 80 * 81 // 2
    seen = set()
    for line in lines:
        y0, y1, lo, hi = map(int, line.split())
        seen.add((y0, y1))
        want = brute(y0, y1)
        got = set(range(lo, hi + 1))
        assert got == want, (y0, y1, lo, hi, sorted(want))
        assert want == set(range(min(want), max(want) + 1)) if want else lo > hi      # contiguous: a range says it all
    assert NONE in seen and all((a, b) in seen for a in range(80) for b in range(a, 80))
    assert brute(*NONE) == set()
    # the numbers of the rule, by hand: V3 row gp reads crop rows 4 gp - 6 .. 4 gp + 9
    assert brute(0, 0) == {0, 1} and brute(79, 79) == {18, 19} and brute(10, 10) == {1, 2, 3, 4} and brute(9, 9) == {0, 1, 2, 3}
    assert brute(27, 52) == set(range(5, 15))


def want_passes(bands):
    total = 20 * len(bands)
    need = [(gp % 20) in brute(*bands[gp // 20]) for gp in range(total)]
    return "".join("1" if any(need[3 * p:3 * p + 3]) else "0" for p in range((total + 2) // 3))


def passes(exe, bands):
    out = run(exe, "passes", *("%d:%d" % b for b in bands))
    assert len(out) == 1
    return out[0]


def test_passes_that_straddle_two_crops(exe):
    # 20 rows per crop, 3 per pass: pass 6 holds rows 18, 19 of crop 0 and row 0 of crop 1; pass 13 row 19 of crop 1 and rows 0, 1 of crop 2
    assert passes(exe, [NONE, NONE, NONE]) == "0" * 20
    assert passes(exe, [NONE, (0, 0), NONE]) == "0" * 6 + "11" + "0" * 12          # crop 1 rows 0, 1 = batch rows 20, 21: passes 6, 7
    assert passes(exe, [(79, 79), NONE, NONE]) == "0" * 6 + "1" + "0" * 13         # crop 0 rows 18, 19: pass 6 alone
    assert passes(exe, [NONE, (79, 79), (0, 0)]) == "0" * 12 + "11" + "0" * 6      # rows 38, 39 and 40, 41: passes 12, 13
    assert passes(exe, [NONE, (78, 78), NONE]) == "0" * 12 + "11" + "0" * 6        # rows 18, 19 of crop 1 again (78 - 9 = 69 > 4 x 17)
    assert passes(exe, [NONE, (73, 73), NONE]) == "0" * 12 + "11" + "0" * 6        # rows 16 .. 19 of crop 1 = batch rows 36 .. 39
    for bands in ([(0, 79)] * 3, [(40, 40), NONE, (3, 70)], [NONE, (5, 5), (74, 79)]):
        assert passes(exe, bands) == want_passes(bands)


def test_the_last_partial_pass(exe):
    # 1 crop: 20 rows = 6 passes of 3 and one of 2 (rows 18, 19); 2 crops: 40 rows, the last pass holds row 39 alone
    assert passes(exe, [NONE]) == "0000000"
    assert passes(exe, [(79, 79)]) == "0000001"
    assert passes(exe, [(0, 79)]) == "1111111"
    assert passes(exe, [NONE, (79, 79)]) == "0" * 12 + "11"
    assert passes(exe, [NONE, (66, 66)]) == want_passes([NONE, (66, 66)])
    assert passes(exe, [NONE, (66, 66)]).endswith("10")                             # 66 + 6 = 72: rows up to 18, row 19 = the last pass is not needed


def test_random_batches(exe):
    rng = random.Random(3)
    for _ in range(40):
        bands = []
        for _ in range(rng.randint(1, 9)):
            if rng.random() < 0.3:
                bands.append(NONE)
            else:
                a = rng.randint(0, 79)
                bands.append((a, rng.randint(a, 79)))
        assert passes(exe, bands) == want_passes(bands), bands


def test_the_switch_is_bit_27_of_the_geometry_word(exe):
    assert run(exe, "plan", 0, 3200) == ["chain=0 skip=1"]
    assert run(exe, "plan", 1 << 27, 3200) == ["chain=0 skip=0"]
    assert run(exe, "plan", 1 << 29, 1) == ["chain=0 skip=1"]
    assert run(exe, "plan", 1 << 29 | 1 << 27, 1) == ["chain=0 skip=0"]
    for geom, n in ((0, 3199), (1 << 30, 12800), (1 << 28, 12800), (1, 12800)):      # every other chain: nothing to skip
        assert run(exe, "plan", geom, n)[0].endswith("skip=0") and not run(exe, "plan", geom, n)[0].startswith("chain=0")
