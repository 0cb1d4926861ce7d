// cnn_skip3.h -- which row pairs of conv3's output depend on which rows of an 80 x 80 identity crop, and how the listed form of k_conv5_wpair
// (cnn_conv3p.h) packs the pairs that must be computed into passes.  Pure constexpr, no device code and no HIP: the device kernels
// (cnn_skip_kernels.h) and tests/cpp/test_cnn_skip3.cpp read the same functions.
//
// conv3 is the same kind of layer as conv1 and conv2 (cnn_skip.h): pooled output row q -- a ROW PAIR of the kernel, conv rows 2q and 2q + 1 --
// reads the V3 rows skip_layer_lo(q) .. skip_layer_hi(q).  A pair all of whose V3 rows are rows the rule of cnn_skip.h calls empty equals, bit
// for bit, the same pair of the all-zero crop's act3 (Net::act3e, made once per loaded network): such a V3 row holds the empty image's bits
// whether k_conv12_rs computed it or k_v3_fill copied it, the rows outside the crop are the zero row either way, and the kernel's arithmetic per
// output element does not depend on the pass, tile or lane it lands in.
#pragma once
#include "cnn_skip.h"

namespace trexhip {

struct Skip3Geom {
    static constexpr int PAIRS = SkipGeom::V3_ROWS / SkipGeom::POOL;        // row pairs per crop (10)
    static constexpr int SLOTS = 6;                                         // row pairs per listed pass: 60 of the kernel's 64 tiles
    static constexpr int RUNS = 2;                                          // runs (one crop's consecutive pairs) per listed pass
    static constexpr int HALO = skip_layer_hi(0) - (SkipGeom::POOL - 1);    // V3 rows a run reads above its first and below its last conv row (2)
    static constexpr int NR = SkipGeom::POOL * SLOTS + 2 * HALO * RUNS;     // V3 rows a listed pass can stage (20: the dense kernel's NR)
    static constexpr int SPAN = 0xfff0;                                     // pairs between a pass's first and last: offsets inside a pass stay below 2^31
    static constexpr int BLOCK = 32;                                        // crops packed by one thread; a pass never holds pairs of two blocks
    static constexpr int BLOCK_PASSES = (BLOCK * PAIRS + SLOTS - 1) / SLOTS + BLOCK + 1;   // full passes + passes closed by a third run + the last
    static constexpr int DESC = 16;                                         // words of a pass's descriptor
    static_assert(PAIRS == 10 && HALO == 2 && NR == 20, "pair q reads V3 rows 2q - 2 .. 2q + 3");
    static_assert((long long)(SPAN + SLOTS) * SkipGeom::POOL * 10240 < (1ll << 31), "V3 byte distance inside a pass");
};

// the row pairs of a crop that must be computed; none: lo > hi
struct SkipPairs { int lo, hi; };

TREXHIP_HD constexpr SkipPairs skip3_pairs(const SkipBand b) {
    using G = Skip3Geom;
    const SkipRows r = skip_rows(b);
    if (r.lo > r.hi) return {1, 0};
    // skip_layer_hi(q) >= r.lo  and  skip_layer_lo(q) <= r.hi
    const int off_hi = skip_layer_hi(0), off_lo = -skip_layer_lo(0);
    const int lo = r.lo <= off_hi ? 0 : (r.lo - off_hi + SKIP_POOL - 1) / SKIP_POOL;
    const int hi = (r.hi + off_lo) / SKIP_POOL;
    return {lo, hi < G::PAIRS - 1 ? hi : G::PAIRS - 1};
}

// a listed pass while it is filled: n pairs from `runs` runs; run r = the pairs gp0[r] .. gp0[r] + len[r] - 1 (global numbering crop * PAIRS + q)
struct Skip3Pass { int n, runs, gp0[Skip3Geom::RUNS], len[Skip3Geom::RUNS]; };

// the pairs gp .. gp + len - 1 of one crop go into the pass being filled and the passes behind it; emit(index, pass) takes every pass that closes.
// A pass closes when it is full, when a third run would begin, or when the next run lies more than SPAN pairs behind its first one
template <class E>
TREXHIP_HD constexpr void skip3_add_run(Skip3Pass& p, int& passes, int gp, int len, E&& emit) {
    using G = Skip3Geom;
    while (len > 0) {
        if (p.n == G::SLOTS || p.runs == G::RUNS || (p.runs && gp - p.gp0[0] > G::SPAN)) { emit(passes, p); ++passes; p = Skip3Pass{}; }
        const int take = len < G::SLOTS - p.n ? len : G::SLOTS - p.n;
        if (p.runs == 0) { p.gp0[0] = gp; p.len[0] = take; }         // (no index that is a variable: the pass stays in registers on the device)
        else { p.gp0[1] = gp; p.len[1] = take; }
        ++p.runs; p.n += take; gp += take; len -= take;
    }
}
template <class E>
TREXHIP_HD constexpr void skip3_flush(Skip3Pass& p, int& passes, E&& emit) {
    if (p.n) { emit(passes, p); ++passes; p = Skip3Pass{}; }
}

// the V3 rows (batch numbering crop * V3_ROWS + y) a run stages: its conv rows and the halo, clipped to the crop
struct Skip3Rows { int row0, n; };
TREXHIP_HD constexpr Skip3Rows skip3_run_rows(const int gp0, const int len) {
    using G = Skip3Geom;
    const int crop = gp0 / G::PAIRS, q0 = gp0 - crop * G::PAIRS, q1 = q0 + len - 1;
    const int lo = skip_layer_lo(q0) > 0 ? skip_layer_lo(q0) : 0;
    const int hi = skip_layer_hi(q1) < SkipGeom::V3_ROWS - 1 ? skip_layer_hi(q1) : SkipGeom::V3_ROWS - 1;
    return {crop * SkipGeom::V3_ROWS + lo, hi - lo + 1};
}

// What the kernel reads of a pass, DESC words:
//   0  first staged V3 row of run A        1  rows of run A          2  V3 rows between the end of run A's rows and run B's first (>= 0)
//   3  rows of both runs (<= NR)           4  first pair of the pass 5  pairs from the first to the last of the pass (the act3 range it stores to)
//   8 + s, s < SLOTS: pair slot s = (pair - first pair) << 16 | q << 8 | LDS row slot of the pair's even conv row (1 ..); idle: 0xffff << 16 | 1
enum : int { S3_ROW0 = 0, S3_NA = 1, S3_GAP = 2, S3_ROWS = 3, S3_GP0 = 4, S3_SPAN = 5, S3_SLOT = 8 };
static constexpr int S3_IDLE = 0xffff;
// (every index into d is a constant once the loops are unrolled: on the device the words stay in registers)
TREXHIP_HD constexpr void skip3_describe(const Skip3Pass& p, int (&d)[Skip3Geom::DESC]) {
    using G = Skip3Geom;
    const bool two = p.runs > 1;
    const int la = p.len[0], lb = two ? p.len[1] : 0, ga = p.gp0[0], gb = two ? p.gp0[1] : ga + la;
    const Skip3Rows a = skip3_run_rows(ga, la);
    const Skip3Rows b = two ? skip3_run_rows(gb, lb) : Skip3Rows{a.row0 + a.n, 0};
    for (int i = 0; i < G::DESC; ++i) d[i] = 0;
    d[S3_ROW0] = a.row0; d[S3_NA] = a.n; d[S3_GAP] = b.row0 - (a.row0 + a.n); d[S3_ROWS] = a.n + b.n;
    d[S3_GP0] = ga; d[S3_SPAN] = (two ? gb + lb : ga + la) - ga;
    for (int s = 0; s < G::SLOTS; ++s) {
        const bool in_a = s < la, in_b = !in_a && s - la < lb;
        const int gp = in_a ? ga + s : gb + (s - la);
        const int slot = 1 + (in_a ? 0 : a.n) + SkipGeom::POOL * gp - (in_a ? a.row0 : b.row0);
        d[S3_SLOT + s] = in_a || in_b ? (gp - ga) << 16 | (gp % G::PAIRS) << 8 | slot : S3_IDLE << 16 | 1;
    }
}

// the words of Net::d_skip that belong to the listed conv3 (the others: cnn_skip_kernels.h)
enum : int {
    SK3_PAIRS = 8,           // row pairs of the last call's batch
    SK3_LISTED = 9,          // row pairs listed
    SK3_PASSES = 10,         // listed passes
    SK3_FILLED = 11,         // act3 row pairs filled from the empty crop's
    SK3_USE = 12,            // non-zero: the listed form of k_conv5_wpair runs, zero: the dense one
    SK3_EMPTY_CTR = 13,      // the pass counter of the run that made the empty crop's act3
    SK3_LAST = SK3_EMPTY_CTR
};

// listed passes against the dense kernel's: the listed form runs when  listed * FACTOR_NUM < dense * FACTOR_DEN.  The factor is what a listed
// pass costs in dense passes, measured on the benchmark's crops under a kernel trace (profiles/conv3_listed_pairs.txt): 3583 us for 31378 listed
// passes against 4523 us for the dense kernel's 40000 = 1.010.  Noise crops (every pair listed: 1.067 times the dense passes) stay dense,
// the benchmark's crops (0.784) are listed; what the list and fill kernels cost beside that is the same either way
static constexpr int SKIP3_FACTOR_NUM = 101, SKIP3_FACTOR_DEN = 100;
TREXHIP_HD constexpr bool skip3_use_list(const long long listed, const long long dense) {
    return listed * SKIP3_FACTOR_NUM < dense * SKIP3_FACTOR_DEN;
}

}  // namespace trexhip
