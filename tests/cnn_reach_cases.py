"""Inputs of tests/test_cnn_reach_gpu.py and tests/test_cnn_reach_inputs.py: batches of 25600 crops and more, every row of which has an expected
value, because every crop is one of a pool of P = 509 crops.  numpy only; no device, no oracle.

The pool (pool()): 460 of weights.synthetic_crops (9 .. 59 non-zero rows), 19 bands of 6 .. 20 rows cut out of further ones, 10 crops with one
pixel in row 0, 9, 10, 21, 22, 40, 58, 69, 70, 79 (the rows where skip_rows / skip3_pairs change their answer at both crop edges), 4 all-zero
crops and 16 noise crops.  509 is prime; 493, the crops that are not noise, is 17 x 29: neither shares a factor with a tile (64), a block of the
pair list (32 crops), a workgroup of it (8192 crops), a conv2 pass (3 V3 rows) or a listed pass (6 pairs).

A batch (batch(kind, n)) is pool[idx]; idx is returned, so the expected row of crop i is the pool's row idx[i].
    "N"   the 16 noise crops, tiled: every pair is listed, the dense conv3 runs, nothing is filled
    "S"   idx[i] = the (i mod 493)-th crop that is not noise, then the overrides below: the listed conv3 runs
    "S2"  S with both sides of the image switch populated
    "M"   N, with the crops of S at the positions of the overrides: conv2 skips their background passes, conv3 stays dense, k_v3_fill copies

The overrides of S and the structure each serves (V3 row of the batch = 20 crop + y, 10240 bytes each; the allocation holds the empty crop's image
in rows 0 .. 19, V3 row r in row 20 + r, the image again behind the last V3 row):
  * the image switch.  A listed pass that reads an image row bases its resource at the front image while 20 + last + 1 <= 393216
    (0xF0000000 / 10240), last its last V3 row.  Crop c's rows are 20 c .. 20 c + 19: crop 19658 ends at row 393179, 20 + 393179 + 1 = 393200:
    always front.  Crop 19660 starts at row 393200, 20 + 393200 + 1 > 393216: always back.  (Crop 19659, rows 393180 .. 393199, is front up to
    last = 393195, its row 15.)  The 32-crop block 614 = crops 19648 .. 19679 straddles the switch, and a pass never leaves its block.
      S:   crop 19648 = one pixel in row 9 (pairs 0 .. 2), 19649 .. 19678 empty, 19679 = one pixel in row 70 (pairs 7 .. 9): ONE pass of two runs,
           its first row 392960 in reach of the front image, its last 393599 not: it bases at its own first row and reads the back image
           638 rows further for run B than for run A.
      S2:  19650 .. 19658 and 19660 .. 19670 are synthetic crops in addition (19659 stays empty): passes that read image rows on either side,
           and crop 19658 is chosen so that one pass holds its last pairs and crop 19660's first: a front-only and a back-only crop in one pass.
  * 4 GB.  2^32 / 10240 = 419430.4: V3 row 419430 = crop 20971, row 10, straddles byte 2^32 from V3's first.  Crops 20965 .. 20978 are synthetic
    crops: own rows, halo rows and image rows of passes on both sides and across.
  * the workgroups of k_pair_count / k_pair_list hold 256 threads x 32 crops = 8192 crops: crops 8190 .. 8194, 16382 .. 16386, 24574 .. 24578
    are synthetic crops -- the last block of one workgroup and the first of the next, whose first pass takes its index from the sum of the
    workgroups in front.
  * the batch's edges: crops 0, n - 1 and n - 2 are synthetic crops, crop n - 3 is empty.
An override outside the batch (n below it) is left out.
"""
import functools
import numpy as np
from trex_amd import weights

P = 509
N_SYNTH, N_BANDS, N_NOISE, N_ZERO = 460, 19, 16, 4
PIXEL_ROWS = (0, 9, 10, 21, 22, 40, 58, 69, 70, 79)
V3_ROWS, V3_ROWB, PAIRS, SLOTS, BLOCK, GROUP, RPP, SPAN = 20, 10240, 10, 6, 32, 8192, 3, 0xfff0
REACH_ROWS = 0xF0000000 // V3_ROWB                           # 393216
SWITCH_BLOCK = (REACH_ROWS // V3_ROWS) // BLOCK              # 614: the block of crop 19660
STRADDLE_ROW = (1 << 32) // V3_ROWB                          # 419430
STRADDLE_CROP = STRADDLE_ROW // V3_ROWS                      # 20971
LAST_FRONT, FIRST_BACK = 19658, 19660
PAIRB = 10 * 128 * 4                                         # bytes of one row pair of act3
LIMITS = (4368.0, 4368.0, 65520.0)                           # fp16x3 range: behind conv1, in front of conv3, in front of fc1
BAND = 0.005


@functools.lru_cache(maxsize=None)
def _pool():
    synth = weights.synthetic_crops(N_SYNTH, 9001)
    # bands cut as sparse() of test_cnn_v3_direct_gpu.py cuts them; the ones that miss their blob altogether are left out
    src = weights.synthetic_crops(60, 9002)
    bands = []
    for i in range(60):
        y0 = (7 * i) % 60
        c = np.zeros_like(src[i])
        c[y0:y0 + 6 + i % 15] = src[i, y0:y0 + 6 + i % 15]
        if c.any() and len(bands) < N_BANDS:
            bands.append(c)
    assert len(bands) == N_BANDS
    pixels = np.zeros((len(PIXEL_ROWS), 80, 80, 1), np.uint8)
    for k, r in enumerate(PIXEL_ROWS):
        pixels[k, r, (37 * r + 11) % 80, 0] = 255
    noise = np.random.default_rng(9003).integers(0, 256, (N_NOISE, 80, 80, 1)).astype(np.uint8)
    zero = np.zeros((N_ZERO, 80, 80, 1), np.uint8)
    crops = np.concatenate([synth, np.stack(bands), pixels, zero, noise])
    kinds = np.array(["synth"] * N_SYNTH + ["band"] * N_BANDS + ["pixel"] * len(PIXEL_ROWS) + ["zero"] * N_ZERO + ["noise"] * N_NOISE)
    # one fixed shuffle: the kinds lie scattered over the pool and so over every batch
    order = np.random.default_rng(9004).permutation(P)
    crops, kinds = np.ascontiguousarray(crops[order]), kinds[order]
    crops.setflags(write=False); kinds.setflags(write=False)
    assert crops.shape == (P, 80, 80, 1)
    return crops, kinds


def pool():
    """-> the 509 crops (uint8, read-only)"""
    return _pool()[0]


def kinds():
    """-> the kind of every pool crop: "synth", "band", "pixel", "zero", "noise" """
    return _pool()[1]


def ids(*which):
    return np.flatnonzero(np.isin(kinds(), which))


def pixel_id(row):
    """the pool crop whose one pixel lies in `row`"""
    hit = [int(i) for i in ids("pixel") if pool()[i, row].any()]
    assert len(hit) == 1
    return hit[0]


def overrides(n, variant="S"):
    """-> {crop of the batch: pool crop} of the structural positions inside a batch of n crops"""
    synth, zero = ids("synth"), int(ids("zero")[0])
    pick = lambda i: int(synth[(7 * i) % len(synth)])
    o = {}
    b0 = SWITCH_BLOCK * BLOCK
    o[b0] = pixel_id(9)
    for c in range(b0 + 1, b0 + BLOCK - 1):
        o[c] = zero
    o[b0 + BLOCK - 1] = pixel_id(70)
    if variant == "S2":
        for c in list(range(b0 + 2, LAST_FRONT + 1)) + list(range(FIRST_BACK, FIRST_BACK + 11)):
            o[c] = pick(c)
        # crop 19658 is the first synthetic crop (counting on from its pick) that leaves a pass open for crop 19660's first pairs
        _, prs = pool_rules()
        for k in range(len(synth)):
            o[LAST_FRONT] = int(synth[(7 * LAST_FRONT + k) % len(synth)])
            block = listed_passes([prs[o[c]] for c in range(b0, b0 + BLOCK)])
            if any(p[0][0] // PAIRS == LAST_FRONT - b0 and p[-1][0] // PAIRS == FIRST_BACK - b0 for p in block):
                break
        else:
            raise AssertionError("no synthetic crop leaves a pass open at the image switch")
    for c in range(STRADDLE_CROP - 6, STRADDLE_CROP + 8):
        o[c] = pick(c)
    for g in range(GROUP, n + 2, GROUP):
        for c in range(g - 2, g + 3):
            o[c] = pick(c)
    for c in (0, n - 2, n - 1):
        o[c] = pick(c)
    o[n - 3] = zero
    return {c: v for c, v in o.items() if 0 <= c < n}


@functools.lru_cache(maxsize=None)
def indices(kind, n):
    """-> idx (int64, read-only): crop i of the batch is pool crop idx[i]"""
    assert kind in ("S", "S2", "N", "M")
    base = ids("noise") if kind in ("N", "M") else ids("synth", "band", "pixel", "zero")
    idx = base[np.arange(n) % len(base)].astype(np.int64)
    if kind != "N":
        for c, v in overrides(n, "S2" if kind == "S2" else "S").items():
            idx[c] = v
    idx.setflags(write=False)
    return idx


def batch(kind, n):
    """-> (crops (n, 80, 80, 1) uint8, idx)"""
    idx = indices(kind, n)
    return pool()[idx], idx


# ---- what the skip rules say about a batch, restated in plain Python (the rules: trex_amd/csrc/cnn_skip.h, cnn_skip3.h) ----

def band_of(crop):
    rows = np.flatnonzero(crop.reshape(80, -1).any(1))
    return (int(rows[0]), int(rows[-1])) if len(rows) else None


def v3_rows_of(crop):
    """the V3 rows of a crop that read one of its non-zero rows: V3 row r reads the crop rows 4 r - 6 .. 4 r + 9"""
    b = band_of(crop)
    return [r for r in range(V3_ROWS) if b and b[0] <= 4 * r + 9 and b[1] >= 4 * r - 6]


def pairs_of(crop):
    """the row pairs of a crop that read one of its non-zero rows: pair q reads the crop rows 8 q - 14 .. 8 q + 21 (pairs_of, test_cnn_skip3_gpu.py)"""
    b = band_of(crop)
    return [q for q in range(PAIRS) if b and b[0] <= 8 * q + 21 and b[1] >= 8 * q - 14]


@functools.lru_cache(maxsize=None)
def pool_rules():
    """-> per pool crop: (first V3 row, V3 rows), (first pair, pairs); rows and pairs are consecutive"""
    rows, prs = [], []
    for c in pool():
        r, q = v3_rows_of(c), pairs_of(c)
        assert r == list(range(r[0], r[-1] + 1)) if r else True
        assert q == list(range(q[0], q[-1] + 1)) if q else True
        rows.append((r[0], len(r)) if r else (0, 0))
        prs.append((q[0], len(q)) if q else (0, 0))
    return np.array(rows), np.array(prs)


def listed_passes(runs):
    """the passes the listed conv3 packs the runs [(first pair, pairs)] of consecutive crops into: six pairs to a pass, of two runs at most, a
    run being the consecutive pairs of one crop in one pass; no pass holds pairs of two 32-crop blocks.  -> [[(global first pair, pairs), ...]]"""
    out = []
    for b0 in range(0, len(runs), BLOCK):
        cur, n = [], 0
        for c in range(b0, min(b0 + BLOCK, len(runs))):
            gp, left = c * PAIRS + int(runs[c][0]), int(runs[c][1])
            while left > 0:
                if n == SLOTS or len(cur) == 2 or (cur and gp - cur[0][0] > SPAN):
                    out.append(cur); cur, n = [], 0
                take = min(left, SLOTS - n)
                cur.append((gp, take))
                n += take; gp += take; left -= take
        if cur:
            out.append(cur)
    return out


def dense_passes(n):
    """the dense conv3's passes: 64 of a crop's 100 tiles each"""
    return (n * 100 + 63) // 64


@functools.lru_cache(maxsize=None)
def expected_stats(kind, n):
    """-> dict: what skip_stats() and skip3_stats() must say after the batch, from the inputs alone"""
    idx = indices(kind, n)
    rows, prs = pool_rules()
    r, q = rows[idx], prs[idx]
    need = np.zeros(n * V3_ROWS, bool)
    for c in np.flatnonzero(r[:, 1]):
        need[c * V3_ROWS + r[c, 0]:c * V3_ROWS + r[c, 0] + r[c, 1]] = True
    n_pass = (n * V3_ROWS + RPP - 1) // RPP
    padded = np.zeros(n_pass * RPP, bool)
    padded[:len(need)] = True
    listed2 = np.zeros(n_pass * RPP, bool)
    listed2[:len(need)] = need
    passes2 = listed2.reshape(n_pass, RPP).any(1)
    rows_listed = int(padded.reshape(n_pass, RPP)[passes2].sum())
    listed = int(q[:, 1].sum())
    passes = len(listed_passes(q))
    use = passes < dense_passes(n)
    return {"skip": (n_pass, int(passes2.sum()), (n * V3_ROWS - rows_listed) * V3_ROWB),
            "pairs": n * PAIRS, "listed": listed, "list_passes": passes, "dense_passes": dense_passes(n), "use_list": use,
            "skip3": (n * PAIRS, listed, passes if use else 0, (n * PAIRS - listed) * PAIRB if use else 0)}
