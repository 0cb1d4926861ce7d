"""Which (crop, split-K plane) rows the listed fc1 computes (skip3_fc1_listed, trex_amd/csrc/cnn_skip3.h) and the per-plane crop lists it walks, on
the CPU: tests/cpp/test_fc1_list.cpp prints what the header's rule says and what a host restatement of k_fc1_list's compaction makes of a batch
of bands; this file derives both from a brute-force propagation of dependence, layer by layer on sets of rows (three times: 5 x 5 'same'
convolution, then 2 x 2 max-pool; 80 -> 40 -> 20 -> 10 rows), without the rule's formulas.  The program is built twice, plainly and with the
address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NONE = (80, -1)
FULL = (0, 79)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fc1_list") / ("test_fc1_list_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_fc1_list.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


def conv_rows(dirty, rows):
    return {y for y in range(rows) if any(0 <= y + k < rows and y + k in dirty for k in (-2, -1, 0, 1, 2))}


def pool_rows(dirty, rows):
    return {r for r in range(rows // 2) if 2 * r in dirty or 2 * r + 1 in dirty}


_PAIR_ROWS = {}


def pair_rows(y0, y1):
    """the rows of act3 (= fc1's split-K planes) of a crop whose non-zero rows lie in y0 .. y1, by propagation"""
    if (y0, y1) not in _PAIR_ROWS:
        d = set(range(y0, y1 + 1))
        for rows in (80, 40, 20):
            d = pool_rows(conv_rows(d, rows), rows)
        _PAIR_ROWS[(y0, y1)] = d
    return _PAIR_ROWS[(y0, y1)]


@pytest.mark.parametrize("all_", [0, 1])
def test_rule_of_every_band_and_plane(exe, all_):
    lines = run(exe, "rule", all_)
    assert len(lines) == 3241
    seen = set()
    for line in lines:
        y0, y1, mask = map(int, line.split())
        seen.add((y0, y1))
        want = set(range(10)) if all_ else pair_rows(y0, y1)
        assert {q for q in range(10) if mask >> q & 1} == want and mask < 1 << 10, (y0, y1, mask, sorted(want))
    assert NONE in seen and len(seen) == 3241
    if not all_:
        assert pair_rows(*NONE) == set() and pair_rows(*FULL) == set(range(10)) and pair_rows(40, 40) == {3, 4, 5, 6}


def lists(exe, bands, all_=0):
    out = run(exe, "lists", all_, *("%d:%d" % b for b in bands))
    assert len(out) == 10
    got = []
    for q, line in enumerate(out):
        head, _, tail = line.partition(":")
        assert int(head.split()[0]) == q
        crops = list(map(int, tail.split()))
        assert len(crops) == int(head.split()[1])
        got.append(crops)
    return got


def want_lists(bands, all_=0):
    return [[c for c, b in enumerate(bands) if all_ or q in pair_rows(*b)] for q in range(10)]


def test_all_empty_and_all_noise(exe):
    for n in (1, 63, 64, 65, 200):
        assert lists(exe, [NONE] * n) == [[]] * 10
        assert lists(exe, [FULL] * n) == [list(range(n))] * 10
        assert lists(exe, [NONE] * n, all_=1) == [list(range(n))] * 10       # the range word set: every crop in every plane


def test_one_pixel_crops_in_every_row(exe):
    bands = [(r, r) for r in range(80)]
    got = lists(exe, bands)
    assert got == want_lists(bands)
    # by hand: plane q reads crop rows 8 q - 14 .. 8 q + 21
    assert got[0] == list(range(0, 22)) and got[9] == list(range(58, 80)) and got[4] == list(range(18, 54))
    mixed = [NONE, (0, 0), FULL, (79, 79), NONE, (40, 40)]
    assert lists(exe, mixed) == want_lists(mixed)
    assert lists(exe, mixed)[5] == [2, 5] and lists(exe, mixed)[0] == [1, 2]


def test_lengths_at_the_tile_edges_in_one_plane(exe):
    """plane 0 is listed by the crops with a pixel in rows 0 .. 21 and by no crop with its pixel in row 40: lengths 0, 1, 127, 128, 129 of plane 0
    among crops that plane 4 always lists, in batches that are no multiple of the 64 crops of a bit-map word"""
    for ln in (0, 1, 127, 128, 129):
        bands = []
        for i in range(ln):                      # a listed crop, then a gap of i % 3 crops that plane 0 does not list
            bands += [(i % 22, i % 22)] + [(40, 40)] * (i % 3)
        bands += [(40, 40)] * 5
        got = lists(exe, bands)
        assert got == want_lists(bands)
        assert len(got[0]) == ln and len(got[4]) >= len(bands) - ln and got[9] == []
        assert got[0] == sorted(got[0]) and all(bands[c] != (40, 40) for c in got[0])


def test_random_batches(exe):
    import random
    rng = random.Random(11)
    for _ in range(20):
        bands = []
        for _ in range(rng.randint(1, 300)):
            if rng.random() < 0.15:
                bands.append(NONE)
            else:
                y0 = rng.randint(0, 79)
                bands.append((y0, rng.randint(y0, 79)))
        assert lists(exe, bands) == want_lists(bands)


def test_plan_and_the_switch(exe):
    RS, OFF = 1 << 29, 1 << 24
    assert run(exe, "plan", 0, 3200) == ["fc1_listed=1 fc1=2 head=1 fill=200"]
    assert run(exe, "plan", 0, 25600) == ["fc1_listed=1 fc1=2 head=1 fill=1600"]
    assert run(exe, "plan", OFF, 25600) == ["fc1_listed=0 fc1=2 head=1 fill=1600"]
    assert run(exe, "plan", RS, 1025) == ["fc1_listed=1 fc1=2 head=1 fill=65"]
    assert run(exe, "plan", RS | OFF, 1025) == ["fc1_listed=0 fc1=2 head=1 fill=65"]
    assert run(exe, "plan", RS, 1024) == ["fc1_listed=0 fc1=1 head=0 fill=64"]           # small batches: k_fc1_split<1>, k_head_small and the fill
    assert run(exe, "plan", RS, 1) == ["fc1_listed=0 fc1=1 head=0 fill=1"]
    for geom, n in ((0, 3199), (1 << 26, 3200), (1 << 27, 3200), (1 << 28, 12800), (1 << 30, 12800), (1, 12800)):
        assert run(exe, "plan", geom, n)[0].startswith("fc1_listed=0 "), (geom, n)
