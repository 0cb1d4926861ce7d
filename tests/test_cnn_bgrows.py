"""The background rows of the windowed conv1+conv2 (trex_amd/csrc/cnn_skipx.h: skipx_v2_rows, rs_round) on the CPU: tests/cpp/test_cnn_bgrows.cpp
prints what the header says, and this file holds it to a brute-force scan of the crop rows each V2 row reads, without the header's formulas:
   V2 row y (conv1's pooled row, 40 per crop) reads the crop rows 2 y - 2 .. 2 y + 3 that exist; it is a background row where none of them
   holds a non-zero byte
   V3 row r (conv2's pooled row, 20 per crop) reads the V2 rows 2 r - 2 .. 2 r + 3 that exist; a windowed pass is up to 4 consecutive V3 rows
The program is built twice, plainly and with the address and undefined-behaviour sanitizers; both are stand-alone executables."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
RPP, CHUNK = 4, 8
BANDS = 80 * 81 // 2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_bgrows") / ("test_cnn_bgrows_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "test_cnn_bgrows.cpp"), "-o", path])
    return path


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def blob_rows(y0, y1):
    """the V2 rows with a non-zero crop row under them, by scanning the crop rows each one reads"""
    return {y for y in range(40) if any(0 <= r < 80 and y0 <= r <= y1 for r in range(2 * y - 2, 2 * y + 4))}


def needed_v3(y0, y1):
    """the V3 rows that read a V2 row of blob_rows"""
    v2 = blob_rows(y0, y1)
    return {r for r in range(20) if any(y in v2 for y in range(2 * r - 2, 2 * r + 4))}


def rounds(exe, what):
    """{(y0, y1): [(k, 'f' | 't', lo, hi, clo, chi, chunks, ...)]} in the order printed"""
    out = {}
    for line in run(exe, what):
        t = line.split()
        out.setdefault((int(t[0]), int(t[1])), []).append((int(t[2]), t[3], *map(int, t[4:])))
    assert len(out) == BANDS
    return out


@pytest.fixture(scope="module")
def clipped(exe):
    return rounds(exe, "rounds")


def test_v2_rows_of_every_band(exe):
    lines = run(exe, "v2rows")
    assert len(lines) == 1 + BANDS
    none = lines[0].split()
    assert none[0] == "none" and int(none[1]) > int(none[2])
    seen = set()
    for line in lines[1:]:
        y0, y1, lo, hi = map(int, line.split())
        want = blob_rows(y0, y1)
        assert want == set(range(lo, hi + 1)), line              # the scan's rows are one run, and the header names exactly that run
        assert 0 <= lo <= hi <= 39
        seen.add((y0, y1))
    assert len(seen) == BANDS


def test_a_pass_reads_its_rows_and_a_follower_only_the_new_ones(clipped):
    for (y0, y1), rs in clipped.items():
        need = needed_v3(y0, y1)
        lo_v3, hi_v3 = min(need), max(need)
        assert need == set(range(lo_v3, hi_v3 + 1))
        passes = -(-(hi_v3 - lo_v3 + 1) // RPP)
        assert [r[0] for r in rs] == [k for k in range(passes) for _ in "ft"] and [r[1] for r in rs] == ["f", "t"] * passes
        prev_hi = None
        for k in range(passes):
            f, t = rs[2 * k], rs[2 * k + 1]
            r0, rl = lo_v3 + RPP * k, min(lo_v3 + RPP * k + RPP - 1, hi_v3)
            reads = [y for y in range(2 * r0 - 2, 2 * rl + 4) if 0 <= y < 40]
            assert (t[2], t[3]) == (reads[0], reads[-1] + 1), (y0, y1, k)          # a ticket's first pass: every row it reads is new
            assert f[3] == t[3] and f[2] == (t[2] if k == 0 else max(prev_hi, t[2])), (y0, y1, k)
            prev_hi = t[3]
            assert t[-1] == lo_v3 and f[-1] == lo_v3


def test_every_row_read_and_not_made_is_background(clipped):
    left_out = 0
    for (y0, y1), rs in clipped.items():
        blob = blob_rows(y0, y1)
        made_so_far = set()
        for k, how, lo, hi, clo, chi, chunks, stages, _ in rs:
            assert lo <= clo <= chi <= hi or (clo == chi and lo <= hi), (y0, y1, k, how)
            made = set(range(clo, chi))
            assert made <= set(range(lo, hi))
            for y in range(lo, hi):
                if y not in made:
                    assert y not in blob, (y0, y1, k, how, y)                      # not made: nothing but background under it
                    left_out += 1
            assert made <= blob, (y0, y1, k, how)                                # and no background row is made
            if how == "f":
                made_so_far |= made
        # over the crop's passes as one run, every non-background row a pass reads was made, once
        read = set()
        for k, how, lo, hi, *_ in rs:
            read |= set(range(lo, hi))
        assert made_so_far == read & blob
        assert sum(r[5] - r[4] for r in rs if r[1] == "f") == len(made_so_far)
    assert left_out > 0


def test_chunks_follow_the_rows_made(clipped):
    more_than_one = 0
    for (y0, y1), rs in clipped.items():
        for k, how, lo, hi, clo, chi, chunks, stages, _ in rs:
            made = chi - clo
            assert chunks == (1 if made <= CHUNK else -(-made // CHUNK)) and stages == 3 * chunks, (y0, y1, k, how)
            more_than_one += chunks > 1
    assert more_than_one > 0           # a blob that starts in the crop's first rows: 10 rows, two chunks


def test_first_pass_of_a_crop_whose_first_needed_row_is_not_row_0_fits_one_chunk(clipped):
    n = 0
    for (y0, y1), rs in clipped.items():
        for k, how, lo, hi, clo, chi, chunks, stages, need_lo in rs:
            if k == 0 and need_lo > 0:
                assert chi - clo <= CHUNK and chunks == 1, (y0, y1, how)
                n += 1
    assert n > 0


def test_hand_derived_rounds(clipped):
    # a blob in crop rows 30 .. 41: V2 rows 14 .. 21 have a crop row of it under them (2 * 14 + 3 = 31 >= 30, 2 * 21 - 2 = 40 <= 41),
    # V3 rows 6 .. 11 are needed; pass 0 = V3 rows 6 .. 9 reads V2 rows 10 .. 21 and makes 14 .. 21 (8, one chunk); pass 1 = V3 rows 10, 11 reads
    # 18 .. 25, as a follower 22 .. 25 of which none is made; as a ticket's first pass it makes 18 .. 21
    rs = clipped[(30, 41)]
    assert rs[0][:7] == (0, "f", 10, 22, 14, 22, 1) and rs[1][:7] == (0, "t", 10, 22, 14, 22, 1)
    assert rs[2][2:4] == (22, 26) and rs[2][5] - rs[2][4] == 0 and rs[2][6] == 1
    assert rs[3][:7] == (1, "t", 18, 26, 18, 22, 1)
    # a blob over every row: every row is made, the first pass makes 10 rows in two chunks
    rs = clipped[(0, 79)]
    assert rs[0][:7] == (0, "f", 0, 10, 0, 10, 2)
    assert all(r[2:4] == r[4:6] for r in rs)


def test_without_the_rule_every_new_row_is_made(exe):
    for (y0, y1), rs in rounds(exe, "noclip").items():
        for k, how, lo, hi, clo, chi, chunks in rs:
            assert (clo, chi) == (lo, hi) and chunks == (1 if hi - lo <= CHUNK else -(-(hi - lo) // CHUNK))


def test_the_switch(exe):
    assert run(exe, "plan", 0, 3200) == ["skipx=1 bgrows=1"]
    assert run(exe, "plan", 1 << 22, 3200) == ["skipx=1 bgrows=0"]                        # bit 22: windows, every row made
    assert run(exe, "plan", 1 << 23, 3200) == ["skipx=0 bgrows=0"]
    assert run(exe, "plan", 1 << 27, 3200) == ["skipx=0 bgrows=0"]
    assert run(exe, "plan", 1 << 29, 1) == ["skipx=1 bgrows=1"]
    assert run(exe, "plan", 1 << 29 | 1 << 22, 1) == ["skipx=1 bgrows=0"]
    assert run(exe, "plan", 1 << 28, 3200) == ["skipx=0 bgrows=0"]
