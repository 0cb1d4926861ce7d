"""The windowed conv1+conv2's rule in x, its windows, its packing and its barrier count (trex_amd/csrc/cnn_skipx.h) on the CPU:
tests/cpp/test_cnn_skipx.cpp prints what the header says, and this file propagates the dependence by brute force on sets of columns, without
the header's formulas:
   5 x 5 'same' convolution: output column x reads input columns x - 2 .. x + 2 that exist;  2 x 2 max-pool: output column c reads 2 c, 2 c + 1
   crop (80 columns) -> conv -> pool (the 40 V2 columns) -> conv (40 columns of conv2's output); an F(4,5) tile is 4 of those: 10 tiles, each
   reading an 8-column input window
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NONE = (80, -1)
WT, RPP, CHUNK = 8, 4, 8


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_skipx") / ("test_cnn_skipx_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_skipx.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


def conv(dirty, size):
    return {x for x in range(size) if any(0 <= x + k < size and x + k in dirty for k in (-2, -1, 0, 1, 2))}


def pool(dirty, size):
    return {c for c in range(size // 2) if 2 * c in dirty or 2 * c + 1 in dirty}


def tiles_of(x0, x1):
    """the conv2 tiles of a crop whose non-zero columns lie in x0 .. x1, two ways: through conv2's output columns, and through the 8-column
    input window of each tile"""
    v2 = pool(conv(set(range(x0, x1 + 1)), 80), 80)
    out = conv(v2, 40)
    by_output = {t for t in range(10) if any(4 * t + k in out for k in range(4))}
    by_window = {t for t in range(10) if any(c in v2 for c in range(4 * t - 2, 4 * t + 6))}
    assert by_output == by_window
    return by_window


def v3_rows(y0, y1):
    d = pool(conv(set(range(y0, y1 + 1)), 80), 80)
    return pool(conv(d, 40), 40)


def test_tile_range_of_every_column_band(exe):
    lines = run(exe, "tiles")
    assert len(lines) == 1 + 80 * 81 // 2 == 3241
    seen = set()
    for line in lines:
        x0, x1, lo, hi = map(int, line.split())
        seen.add((x0, x1))
        want = tiles_of(x0, x1)
        assert set(range(lo, hi + 1)) == want, (x0, x1, lo, hi, sorted(want))
        assert want == set(range(min(want), max(want) + 1)) if want else lo > hi
    assert NONE in seen and all((a, b) in seen for a in range(80) for b in range(a, 80))
    # the numbers of the rule, by hand: tile t reads crop columns 8 t - 6 .. 8 t + 13
    assert tiles_of(0, 0) == {0} and tiles_of(2, 2) == {0, 1} and tiles_of(13, 13) == {0, 1, 2} and tiles_of(14, 14) == {1, 2}
    assert tiles_of(79, 79) == {9} and tiles_of(73, 73) == {8, 9}


def window(exe, x0, x1, out_of_range=0):
    return int(run(exe, "window", x0, x1, out_of_range)[0])


def test_windows(exe):
    # at t0 = 0 and at the right edge (the window is moved left so that it ends at tile 9)
    assert window(exe, 0, 0) == 0 and window(exe, 0, 50) == 0          # 50 + 6 = 56: tiles 0 .. 7, exactly WT
    assert window(exe, 79, 79) == 2 and window(exe, 30, 79) == 2       # 30 - 13 = 17: tiles 3 .. 9 -> [2, 10)
    # exactly WT tiles wide, and one tile wider: no window
    assert tiles_of(22, 73) == set(range(2, 10)) and window(exe, 22, 73) == 2
    assert tiles_of(21, 73) == set(range(1, 10)) and window(exe, 21, 73) == -1
    assert tiles_of(14, 66) == set(range(1, 10)) and window(exe, 14, 66) == -1
    assert tiles_of(14, 65) == set(range(1, 9)) and window(exe, 14, 65) == 1
    assert window(exe, 0, 57) == 0 and window(exe, 0, 58) == -1       # 58 + 6 = 64: tile 8
    assert window(exe, 0, 79) == -1
    # the empty crop's image is not to be used: no window, however narrow the blob
    assert window(exe, 40, 40, 1) == -1 and window(exe, *NONE, 1) == -1
    # every band: a window holds every tile of the band, lies inside the row, and is refused only for bands wider than WT tiles
    lines = run(exe, "windows")
    assert len(lines) == 80 * 81 // 2
    for line in lines:
        x0, x1, w = map(int, line.split())
        t = tiles_of(x0, x1)
        if len(t) > WT:
            assert w == -1, (x0, x1)
        else:
            assert 0 <= w <= 10 - WT and min(t) >= w and max(t) < w + WT, (x0, x1, w)
    assert window(exe, *NONE) == 0                                     # no blob: a window and no pass


def pack(exe, crop, lo, hi, t0):
    return [tuple(map(int, line.split())) for line in run(exe, "pack", crop, lo, hi, t0)]


def test_packing_of_runs(exe):
    assert pack(exe, 5, 1, 0, 0) == []                                                       # no needed row
    assert [p[:4] for p in pack(exe, 5, 7, 7, 1)] == [(5, 7, 1, 1)]                          # a run of 1 row
    assert [p[:4] for p in pack(exe, 5, 6, 6 + RPP // 2, 2)] == [(5, 6, 3, 2)]               # WR / 2 + 1 conv2 row pairs ... 3 V3 rows: one short pass
    assert [p[:4] for p in pack(exe, 3, 2, 6, 0)] == [(3, 2, 4, 0), (3, 6, 1, 0)]            # WR / 2 + 1 = 5 rows: a full pass and a short one
    assert [p[:4] for p in pack(exe, 0, 0, 1, 0)] == [(0, 0, 2, 0)]                          # touching row 0
    assert [p[:4] for p in pack(exe, 9, 14, 19, 2)] == [(9, 14, 4, 2), (9, 18, 2, 2)]        # touching row 19
    assert [p[:4] for p in pack(exe, 1, 0, 19, 1)] == [(1, 4 * k, 4, 1) for k in range(5)]   # every row
    # the entry round-trips at the largest crop index a batch can have, and entries of different passes differ
    big = pack(exe, (1 << 22) - 1, 0, 19, 2)
    assert [p[:4] for p in big] == [((1 << 22) - 1, 4 * k, 4, 2) for k in range(5)] and len({p[4] for p in big}) == 5 and all(p[4] >= 0 for p in big)
    # every run: consecutive passes of one crop, whole, in order, nothing outside the run
    runs = {}
    for lo, hi, crop, r0, n, t0 in (map(int, line.split()) for line in run(exe, "packs", 7, 1)):
        rows = runs.setdefault((lo, hi), [])
        assert crop == 7 and t0 == 1 and 1 <= n <= RPP and (not rows or r0 == rows[-1] + 1)
        assert not rows or len(rows) % RPP == 0                # only the last pass of a run is short
        rows += list(range(r0, r0 + n))
    assert set(runs) == {(lo, hi) for lo in range(20) for hi in range(lo, 20)}
    assert all(rows == list(range(lo, hi + 1)) for (lo, hi), rows in runs.items())


def full(exe, crops):
    out = run(exe, "full", *("%d:%d:%d:%d" % (b + c) for b, c in crops))
    return out[0], [tuple(map(int, line.split())) for line in out[1:]]


def test_two_lists_no_pass_holds_two_crops(exe):
    wide, narrow = (0, 79), (30, 40)
    # crop 0 windowed (rows 18, 19 from its last rows), crop 1 without a window (row 0 ..): pass 6 holds rows 18, 19 of crop 0 and row 0 of crop 1
    bits, wl = full(exe, [((79, 79), narrow), ((0, 0), wide), (NONE, narrow)])
    assert bits == "0" * 6 + "11" + "0" * 12 and wl == [(0, 18, 2, 2)]
    # the other way round: the full-width pass 6 is needed for crop 0 alone, crop 1's rows 0, 1 are a windowed pass of its own
    bits, wl = full(exe, [((79, 79), wide), ((0, 0), narrow)])
    assert bits == "0" * 6 + "1" + "0" * 7 and wl == [(1, 0, 2, 2)]
    # both windowed: no full-width pass at all; both wide: the aligned passes of the row rule
    bits, wl = full(exe, [((79, 79), narrow), ((0, 0), narrow)])
    assert bits == "0" * 14 and wl == [(0, 18, 2, 2), (1, 0, 2, 2)]
    bits, wl = full(exe, [((79, 79), wide), ((0, 0), wide)])
    assert bits == "0" * 6 + "11" + "0" * 6 and wl == []
    # windowed passes come in crop order and never leave their crop
    crops = [((4 * k, 4 * k + 30), narrow) for k in range(12)]
    bits, wl = full(exe, crops)
    assert set(bits) == {"0"} and [p[0] for p in wl] == sorted(p[0] for p in wl)
    for k in range(12):
        rows = [r for c, r0, n, _ in wl if c == k for r in range(r0, r0 + n)]
        assert rows == sorted(v3_rows(4 * k, 4 * k + 30)) and all(0 <= r < 20 for r in rows)


def test_without_windows_the_full_width_list_is_the_row_rules(exe):
    """the identity the one count / list / fill trio rests on: where no crop has a window (win(crop) == -1), skipx_full_needed is
    skip_pass_needed, pass by pass.  Every band at crops 2, 3 and 4 of a batch of 7 -- its 20 V3 rows begin at the second, the first and the third
    row of a 3-row pass -- between an empty crop and a full one"""
    lines = [line.split() for line in run(exe, "nowin")]
    assert len(lines) == 3 * (1 + 80 * 81 // 2)
    seen = set()
    for at, y0, y1, rows, lists in lines:
        at, y0, y1 = int(at), int(y0), int(y1)
        seen.add((at, y0, y1))
        assert rows == lists, (at, y0, y1)
        # ... and both are the brute-force propagation's: the batch's V3 rows that read a non-zero crop row, three to a pass (47 passes, the last of 2)
        need = {20 * at + r for r in (v3_rows(y0, y1) if y0 <= y1 else ())} | set(range(20 * (at + 1), 20 * (at + 2)))
        assert rows == "".join("1" if any(gp in need for gp in range(3 * p, 3 * p + 3)) else "0" for p in range(47)), (at, y0, y1)
    assert seen == {(at, *b) for at in (2, 3, 4) for b in [NONE] + [(a, b) for a in range(80) for b in range(a, 80)]}
    assert {(20 * at) % 3 for at in (2, 3, 4)} == {0, 1, 2}
    # a batch given on the command line: rows 78, 79 reach V3 rows 18, 19 -- passes 6 (with row 0 of the empty crop behind) and nothing else
    assert run(exe, "nowin", "78:79", "80:-1") == ["0" * 6 + "1" + "0" * 7] * 2


def v2_rows(r0, rows):
    """the V2 rows (of the crop, 0 .. 39) that the V3 rows r0 .. r0 + rows - 1 read: conv2's rows 2 r .. 2 r + 1, each two rows up and down"""
    return {y + k for r in range(r0, r0 + rows) for y in (2 * r, 2 * r + 1) for k in (-2, -1, 0, 1, 2) if 0 <= y + k < 40}


def test_barrier_count_of_every_round(exe):
    lines = [line.split() for line in run(exe, "stages")]
    seen = set()
    for inst, kind, a, b, new, chunks, stages in lines:
        a, b, new, chunks, stages = int(a), int(b), int(new), int(chunks), int(stages)
        seen.add((inst, kind, a, b))
        if inst == "w":
            want = v2_rows(a, b) - (v2_rows(a - RPP, RPP) if kind == "next" else set())
            chunk = CHUNK
        else:            # full width: pass a of a 2-crop batch = the batch's V3 rows 3 a .. 3 a + 2, as many as exist; they may belong to two crops
            def rows_of(p):
                out = set()
                for gp in range(3 * p, min(3 * p + 3, 40)):
                    out |= {40 * (gp // 20) + y for y in v2_rows(gp % 20, 1)}
                return out
            want = rows_of(a) - (rows_of(a - 1) if kind == "next" else set())
            chunk = 6
        assert new == len(want), (inst, kind, a, b, new, sorted(want))
        assert chunks == max(1, -(-new // chunk)) and stages == 3 * chunks
        # a pass behind its predecessor never needs a second chunk; a first pass at most two
        assert chunks == 1 if kind == "next" else chunks <= 2
    assert all(("w", "first", r0, n) in seen for r0 in range(20) for n in range(1, RPP + 1) if r0 + n <= 20)
    assert all(("w", "next", r0, n) in seen for r0 in range(RPP, 20) for n in range(1, RPP + 1) if r0 + n <= 20)
    assert all(("f", "first", p, 0) in seen for p in range(14)) and all(("f", "next", p, 0) in seen for p in range(1, 14))


def test_the_switch_is_bit_23_of_the_geometry_word(exe):
    assert run(exe, "plan", 0, 3200) == ["chain=0 skip=1 skipx=1"]
    assert run(exe, "plan", 1 << 23, 3200) == ["chain=0 skip=1 skipx=0"]
    assert run(exe, "plan", 1 << 27, 3200) == ["chain=0 skip=0 skipx=0"]                  # nothing is skipped at all
    assert run(exe, "plan", 1 << 29, 1) == ["chain=0 skip=1 skipx=1"]
    assert run(exe, "plan", 1 << 29 | 1 << 23, 1) == ["chain=0 skip=1 skipx=0"]
    for geom, n in ((0, 3199), (1 << 30, 12800), (1 << 28, 12800), (1, 12800)):           # every other chain
        assert run(exe, "plan", geom, n)[0].endswith("skipx=0")
