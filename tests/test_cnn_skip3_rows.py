"""Where the listed conv3 takes the V3 rows of its passes from (skip3_row_sources / skip3_row_words, trex_amd/csrc/cnn_skip3.h), on the CPU:
tests/cpp/test_cnn_skip3_rows.cpp prints what the header says for every band as run A and as run B of a pass, and this file propagates the
dependence by brute force, layer by layer on sets of rows, without the rule's formulas (twice: 5 x 5 'same' convolution, then 2 x 2 max-pool;
80 -> 40 -> 20 rows).  A row of a crop is read from V3 exactly when it is in that set; every other row comes from the empty crop's image, never
from V3 -- nothing writes it there.  The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are
stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
IDLE = 0xffff
NR, WORDS, BASE, SHIFT = 20, 32, 31, 18
ROWB = 10240
IMAGE, NONE = 1 << 30, -1
REACH, NUM_RECORDS, OFF_NONE = 0xF0000000, 0xF8000000, 0xFFFF0000
# second crops: runs of 4 (pairs 3 .. 6), 10, 2 at the top, 2 at the bottom, none, 5, 7 (pairs 1 .. 7), 6 (pairs 2 .. 7): with every band in front
# of them and behind them the passes are full of one run, 5 + 1, 4 + 2, 2 + 2 and 1 + 4 closed by a third run, and runs are cut at every length
OTHERS = [(40, 40), (0, 79), (0, 0), (79, 79), (80, -1), (21, 21), (25, 45), (30, 44)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_skip3_rows") / ("test_cnn_skip3_rows_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_skip3_rows.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def conv_rows(dirty, rows):
    return {y for y in range(rows) if any(0 <= y + k < rows and y + k in dirty for k in (-2, -1, 0, 1, 2))}


def pool_rows(dirty, rows):
    return {r for r in range(rows // 2) if 2 * r in dirty or 2 * r + 1 in dirty}


_own = {}


def own_rows(y0, y1):
    """the V3 rows of a crop whose non-zero rows lie in y0 .. y1 that differ from the empty crop's"""
    if (y0, y1) not in _own:
        d = set(range(y0, y1 + 1))
        for rows in (80, 40):
            d = pool_rows(conv_rows(d, rows), rows)
        _own[(y0, y1)] = frozenset(d)
    return _own[(y0, y1)]


def check_line(line, total_rows):
    head, desc, src, w = ([int(x) for x in part.split()] for part in line.split("|"))
    ca, ya0, ya1, cb, yb0, yb1 = head
    assert len(desc) == 16 and len(src) == NR and len(w) == WORDS
    own = {ca: own_rows(ya0, ya1), cb: own_rows(yb0, yb1)}
    row0, na, gap, rows, gp0, span = desc[:6]
    # the source of every slot a listed pair's taps read inside its crop
    read = set()
    for s in desc[8:14]:
        rel, q, slot = (s >> 16) & 0xffff, (s >> 8) & 0xff, s & 0xff
        if rel == IDLE:
            continue
        crop = (gp0 + rel) // 10
        assert crop in own and q == (gp0 + rel) % 10
        for par in (0, 1):
            for ky in range(-2, 3):
                y = 2 * q + par + ky
                if 0 <= y < 20:
                    sl = slot + par + ky
                    assert 1 <= sl <= rows
                    read.add(sl)
                    want = crop * 20 + y if y in own[crop] else IMAGE | y
                    assert src[sl - 1] == want, (line, sl, y)
    assert read == set(range(1, rows + 1))                   # a pass stages no row that no pair of it reads
    # no V3 source outside a crop's own rows, in any slot; nothing behind the pass's rows
    for i, s in enumerate(src):
        if i >= rows:
            assert s == NONE
        elif not s & IMAGE:
            assert s // 20 in own and s % 20 in own[s // 20], (line, i)
            assert s == row0 + i + (gap if i >= na else 0)
    # the words: one resource from allocation row `base` ([0, 20) the image, 20 + r V3 row r, 20 + total + y the image again), a byte offset per slot
    base = w[BASE]
    top = 0
    for i in range(WORDS - 1):
        off = (w[i] + (i << SHIFT)) & 0xffffffff
        s = src[i] if i < NR else NONE
        if s == NONE:
            assert off == OFF_NONE
            continue
        assert off % ROWB == 0 and off + ROWB <= REACH, (line, i, off)
        at = base + off // ROWB
        assert at == 20 + s if not s & IMAGE else at in (s & ~IMAGE, 20 + total_rows + (s & ~IMAGE)), (line, i)
        top = max(top, at)
    assert top < 40 + total_rows
    return rows, any(s != NONE and s & IMAGE for s in src), base


@pytest.mark.parametrize("first,total", [(0, 9), (25591, 25600), (20000, 32000)])
def test_every_band_as_run_a_and_as_run_b(exe, first, total):
    """at the front of a batch, at the end of the benchmark's -- out of the front image's reach, the back image's rows -- and in the middle of
    the largest batch (in thousands) that still reaches an image from everywhere"""
    lines = run(exe, "scan", first, total, *("%d:%d" % b for b in OTHERS))
    assert len(lines) > 2 * 3241
    shapes, bases = set(), set()
    for line in lines:
        rows, image, base = check_line(line, total * 20)
        shapes.add((rows, image))
        bases.add(base == 0)
    assert {r for r, _ in shapes} >= {8, 12, 16, 20} and {i for _, i in shapes} == {False, True}
    assert bases == ({True, False} if first == 0 else {False})


def test_reach():
    """by hand: 0xF0000000 / 10240 = 393216 rows within reach; a pass is at most (0xfff0 + 6) * 2 + 4 = 131056 rows long"""
    assert REACH // ROWB == 393216 and REACH + 4 * 2560 <= NUM_RECORDS <= OFF_NONE and OFF_NONE + 4 * ROWB < 1 << 32


def test_fits_and_plan(exe):
    limit = 2 * 393216 - 40 - 131056 - 1
    assert run(exe, "fits", limit) == ["1"] and run(exe, "fits", limit + 1) == ["0"]
    assert run(exe, "fits", 25600 * 20) == ["1"] and run(exe, "fits", 32000 * 20) == ["1"]
    assert run(exe, "plan", 0, 25600) == ["skip3=1 direct=1"]
    assert run(exe, "plan", 1 << 25, 25600) == ["skip3=1 direct=0"]                   # the copy is kept
    assert run(exe, "plan", 1 << 26, 25600) == ["skip3=0 direct=0"]
    assert run(exe, "plan", 1 << 29, 1) == ["skip3=1 direct=1"]
    assert run(exe, "plan", 0, 40000) == ["skip3=1 direct=0"]                         # 8 GB of V3: out of both images' reach in the middle
