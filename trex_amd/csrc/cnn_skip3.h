// cnn_skip3.h -- which row pairs of conv3's output depend on which rows of an 80 x 80 identity crop, and how the listed form of k_conv5_wpair
// (cnn_conv3p.h) packs the pairs that must be computed into passes.  Pure constexpr, no device code and no HIP: the device kernels
// (cnn_skip_kernels.h) and tests/cpp/test_cnn_skip3.cpp read the same functions.
//
// conv3 is the same kind of layer as conv1 and conv2 (cnn_skip.h): pooled output row q -- a ROW PAIR of the kernel, conv rows 2q and 2q + 1 --
// reads the V3 rows skip_layer_lo(q) .. skip_layer_hi(q).  A pair all of whose V3 rows are rows the rule of cnn_skip.h calls empty equals, bit
// for bit, the same pair of the all-zero crop's act3 (Net::act3e, made once per loaded network): such a V3 row holds the empty image's bits
// whether k_conv12_rs computed it, k_v3_fill copied it or the listed kernel reads it from the image itself (skip3_row_sources), the rows outside the crop are the zero row either way, and the kernel's arithmetic per
// output element does not depend on the pass, tile or lane it lands in.
#pragma once
#include "cnn_skip.h"

namespace trexhip {

constexpr bool S3X_DESC_OK(const int desc, const int slots) { return 8 + slots <= desc && (desc & (desc - 1)) == 0; }
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
    static constexpr int TILES = SkipGeom::V3_ROWS / 4;                     // F(4,5) tiles of a row that a pass computes: all 5
    static_assert(PAIRS == 10 && HALO == 2 && NR == 20, "pair q reads V3 rows 2q - 2 .. 2q + 3");
    static_assert((long long)(SPAN + SLOTS) * SkipGeom::POOL * 10240 < (1ll << 31), "V3 byte distance inside a pass");
};

// ---- the rule in x ----
// conv3 tile t (F(4,5): TILE output columns of the 20-wide map) reads the V3 columns TILE t - KH / 2 .. TILE t + TILE - 1 + KH / 2, V3 column c
// conv2's columns under its pool window, those V2's columns skip_layer_lo .. skip_layer_hi, and a V2 column the crop's columns likewise: two
// layers of cnn_skip.h under the tile's window.  A tile whose whole band of crop columns is background -- in every row its pair reads -- holds
// the empty crop's bits, for the reason cnn_skip.h gives for rows.
struct Skip3XGeom {
    static constexpr int PAIRS = Skip3Geom::PAIRS, RUNS = Skip3Geom::RUNS, HALO = Skip3Geom::HALO, SPAN = Skip3Geom::SPAN, BLOCK = Skip3Geom::BLOCK;
    static constexpr int TILE = 4;                                          // conv3 output columns per tile
    static constexpr int ROW_TILES = SkipGeom::V3_ROWS / TILE;              // 5 per row
    static constexpr int WT3 = 3;                                           // the window: tiles of a row that a windowed pass computes
    static constexpr int TILES = WT3;
    static constexpr int SLOTS = 10;                                        // row pairs per windowed pass: 60 of the kernel's 64 tiles, as in the full-width form
    // V3 rows a windowed pass can stage: two runs of any lengths (a narrow row is 0.6 of a full one, so 29 row slots are 93 KB of LDS where the
    // full-width form's 21 are 112 KB).  Packing the benchmark's crops (800 of them, blocks of 32 crops) on the CPU: 20 or 24 rows give 897
    // passes for the narrow and the wide list together, 28 rows 855, against 985 full-width passes; 40 rows (two whole crops) need a 64-word row
    // table and were not tried
    static constexpr int NR = SkipGeom::POOL * SLOTS + 2 * HALO * RUNS;
    static constexpr int BLOCK_PASSES = (BLOCK * PAIRS + SLOTS - 1) / SLOTS + BLOCK + 1;
    static constexpr int DESC = 32;                                         // 8 + SLOTS words, a power of two
    static constexpr int V3_LO0 = -(SKIP_KH / 2), V3_HI0 = TILE - 1 + SKIP_KH / 2;
    static constexpr int STEP = TILE * SkipGeom::POOL * SkipGeom::POOL, LO0 = skip_layer_lo(skip_layer_lo(V3_LO0)), HI0 = skip_layer_hi(skip_layer_hi(V3_HI0));
    static_assert(STEP == 16 && LO0 == -14 && HI0 == 29, "tile t reads crop columns 16 t - 14 .. 16 t + 29");
    static_assert(SLOTS * 2 * WT3 <= 64 && NR == 28 && S3X_DESC_OK(DESC, SLOTS), "60 of 64 tile slots; the descriptor holds the slots");
    static_assert((long long)(SPAN + SLOTS) * SkipGeom::POOL * 10240 < (1ll << 31), "V3 byte distance inside a pass");
};

// the conv3 tiles of a crop that can differ from the empty crop's, from its first and last non-zero COLUMN (SkipBand's y0, y1 read as x0, x1); none: lo > hi
struct Skip3Tiles { int lo, hi; };
TREXHIP_HD constexpr Skip3Tiles skip3_tiles(const SkipBand b) {
    using X = Skip3XGeom;
    if (b.y0 > b.y1) return {1, 0};
    // STEP t + HI0 >= x0  and  STEP t + LO0 <= x1
    const int lo = b.y0 <= X::HI0 ? 0 : (b.y0 - X::HI0 + X::STEP - 1) / X::STEP;
    const int hi = (b.y1 - X::LO0) / X::STEP;
    return {lo, hi < X::ROW_TILES - 1 ? hi : X::ROW_TILES - 1};
}
// the window [t0, t0 + WT3) of a crop; -1: it has none -- it needs more than WT3 tiles, it has no column band (and no pair to compute), or the
// empty crop's image is not to be used
TREXHIP_HD constexpr int skip3_window(const SkipBand cols, const bool empty_out_of_range) {
    using X = Skip3XGeom;
    if (empty_out_of_range) return -1;
    const Skip3Tiles t = skip3_tiles(cols);
    if (t.lo > t.hi || t.hi - t.lo + 1 > X::WT3) return -1;
    return t.lo < X::ROW_TILES - X::WT3 ? t.lo : X::ROW_TILES - X::WT3;
}

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
// (G: Skip3Geom, the full-width passes, or Skip3XGeom, the windowed ones -- the same rule with their slots)
template <class G = Skip3Geom, class E>
TREXHIP_HD constexpr void skip3_add_run(Skip3Pass& p, int& passes, int gp, int len, E&& emit) {
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
//   8 + s, s < SLOTS: pair slot s = (pair - first pair) << 16 | t0 << 12 | q << 8 | LDS row slot of the pair's even conv row (1 ..); idle: 0xffff << 16 | 1
//   (t0: the first tile of the window of the run's crop, windowed passes only: 0 in a full-width pass)
enum : int { S3_ROW0 = 0, S3_NA = 1, S3_GAP = 2, S3_ROWS = 3, S3_GP0 = 4, S3_SPAN = 5, S3_SLOT = 8, S3_T0_SHIFT = 12, S3_Q_MASK = 0xf, S3_T0_MASK = 0x3 };
static constexpr int S3_IDLE = 0xffff;
// (every index into d is a constant once the loops are unrolled: on the device the words stay in registers)
template <class G = Skip3Geom>
TREXHIP_HD constexpr void skip3_describe(const Skip3Pass& p, int (&d)[G::DESC], const int t0a = 0, const int t0b = 0) {
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
        d[S3_SLOT + s] = in_a || in_b ? (gp - ga) << 16 | (in_a ? t0a : t0b) << S3_T0_SHIFT | (gp % G::PAIRS) << 8 | slot : S3_IDLE << 16 | 1;
    }
}

// Where the staged rows of a listed pass come from.  Only the rows inside skip_rows(band) of a crop -- its OWN rows -- are read from V3: every
// other row of the crop holds the empty image's bits by the rule of cnn_skip.h, and the kernel takes it from that image itself (20 rows that stay
// in every L2) instead of from a copy of it in V3.  Nothing writes the rows of V3 outside the own rows then: they hold what an earlier call, or a
// neighbour's straddling conv2 pass, left there, and must never be read.
//   src[i], i < NR: the source of LDS row slot 1 + i (the numbering of S3_SLOT: run A's rows, run B's behind them)
//     >= 0 and < S3_SRC_IMAGE   V3 row crop * V3_ROWS + y
//     S3_SRC_IMAGE | y          row y of the empty image
//     S3_SRC_NONE               behind the pass's rows: reads zeros
// own_a / own_b: skip_rows of the bands of run A's and run B's crop ({0, V3_ROWS - 1}: every row from V3 -- where k_v3_fill has copied the image)
enum : int { S3_SRC_NONE = -1, S3_SRC_IMAGE = 1 << 30 };
template <class G = Skip3Geom>
TREXHIP_HD constexpr void skip3_row_sources(const Skip3Pass& p, const SkipRows own_a, const SkipRows own_b, int (&src)[G::NR]) {
    const bool two = p.runs > 1;
    const Skip3Rows a = skip3_run_rows(p.gp0[0], p.len[0]);
    const Skip3Rows b = two ? skip3_run_rows(p.gp0[1], p.len[1]) : Skip3Rows{a.row0 + a.n, 0};
    const int ca = p.gp0[0] / G::PAIRS, cb = two ? p.gp0[1] / G::PAIRS : ca;
    for (int i = 0; i < G::NR; ++i) {      // (no index that is a variable but the unrolled i)
        const bool in_a = i < a.n, in_b = !in_a && i - a.n < b.n;
        const int row = in_a ? a.row0 + i : b.row0 + (i - a.n);
        const int y = row - (in_a ? ca : cb) * SkipGeom::V3_ROWS;
        const SkipRows own = in_a ? own_a : own_b;
        src[i] = in_a || in_b ? (y >= own.lo && y <= own.hi ? row : S3_SRC_IMAGE | y) : S3_SRC_NONE;
    }
}

// The sources as the kernel reads them: one buffer resource per pass and a 32-bit byte offset per row slot.  A resource reaches 4 GB forward from
// its base and V3 is 5.2 GB at 25600 crops, so the image lies TWICE in V3's allocation, in front of it and behind it:
//   rows of the allocation:  0 .. V3_ROWS - 1 the image | V3_ROWS + r: V3 row r | V3_ROWS + total + y: the image again
// and a pass starts its resource at the front image where its last row is within reach of that, else at its own first row, from where the back
// image is within reach as long as skip3_direct_fits(total).  A pass that reads no image row starts at its first row (any batch size).
//   w[i], i < NR   byte offset of slot 1 + i's source from the resource's base, minus i << S3_ROW_SHIFT (the lane adds its packed constant
//                  row << S3_ROW_SHIFT | byte in the row and has the offset); none: S3_OFF_NONE, at or behind the resource's S3_NUM_RECORDS
//   w[NR .. 30]    none (the lanes of a staging instruction that cover no row use entry NR)
//   w[31]          the row of the allocation the resource starts at
struct Skip3Reach {
    static constexpr int ROWB = 10240;                                      // bytes of a V3 row (V3_ROWB, cnn_wpre.h)
    static constexpr int WORDS = 32, BASE = 31, ROW_SHIFT = 18;
    static constexpr unsigned REACH = 0xF0000000u;                          // every source byte of a pass lies below this offset
    static constexpr unsigned NUM_RECORDS = 0xF8000000u;                    // of the resource (a unit's 2560-byte step comes off base and size alike)
    static constexpr unsigned OFF_NONE = 0xFFFF0000u;                       // + a byte in the row: still below 2^32, never below NUM_RECORDS
    static constexpr long long REACH_ROWS = REACH / ROWB;
    static constexpr int PASS_ROWS = (Skip3Geom::SPAN + Skip3Geom::SLOTS) * SkipGeom::POOL + 2 * Skip3Geom::HALO;   // first to last row of a pass, at most
    static constexpr int PASS_ROWS_X = (Skip3XGeom::SPAN + Skip3XGeom::SLOTS) * SkipGeom::POOL + 2 * Skip3XGeom::HALO;   // ... of a windowed pass
    static constexpr int TILEB = 32;                                        // bytes of a tile in each of a row's position groups: a window starts t0 * TILEB into them
    static_assert(ROWB * 4 <= (1 << ROW_SHIFT) && Skip3Geom::NR < WORDS - 1 && (Skip3Geom::NR << ROW_SHIFT) > 0, "the packed constant");
    static_assert(Skip3XGeom::NR < WORDS - 1 && (Skip3XGeom::NR << ROW_SHIFT) > 0, "the packed constant, windowed passes");
    static_assert(NUM_RECORDS - 4 * 2560 >= REACH && OFF_NONE >= NUM_RECORDS, "none is out of range in every unit's resource");
};
// can every pass of a batch of `total` V3 rows reach an image?  (a pass out of the front image's reach starts behind row
// REACH_ROWS - V3_ROWS - PASS_ROWS - 1 and needs the back image's last row within REACH_ROWS of it)
TREXHIP_HD constexpr bool skip3_direct_fits(const long long total) {
    using R = Skip3Reach;
    return total <= 2 * R::REACH_ROWS - 2 * SkipGeom::V3_ROWS - R::PASS_ROWS - 1;
}
// ... and every windowed pass (10 pair slots: its rows reach further)
TREXHIP_HD constexpr bool skip3x_direct_fits(const long long total) {
    using R = Skip3Reach;
    return total <= 2 * R::REACH_ROWS - 2 * SkipGeom::V3_ROWS - R::PASS_ROWS_X - 1;
}
// (t0a, t0b: windowed passes -- the first tile of the window of run A's and run B's crop: a row's source starts t0 * TILEB bytes into the row, so
// that the lane's constant, which places the window's tiles at the head of each position group, lands on tile t0's)
template <class G = Skip3Geom>
TREXHIP_HD constexpr void skip3_row_words(const Skip3Pass& p, const SkipRows own_a, const SkipRows own_b, const long long total,
                                          unsigned (&w)[Skip3Reach::WORDS], const int t0a = 0, const int t0b = 0) {
    using R = Skip3Reach;
    constexpr int IMG = SkipGeom::V3_ROWS;
    int src[G::NR] = {};
    skip3_row_sources<G>(p, own_a, own_b, src);
    const bool two = p.runs > 1;
    const Skip3Rows a = skip3_run_rows(p.gp0[0], p.len[0]);
    const Skip3Rows b = two ? skip3_run_rows(p.gp0[1], p.len[1]) : Skip3Rows{a.row0 + a.n, 0};
    const long long last = b.row0 + b.n - 1;                               // the pass's first row is a.row0
    bool image = false;
    for (int i = 0; i < G::NR; ++i) image = image || (src[i] != S3_SRC_NONE && (src[i] & S3_SRC_IMAGE));
    const bool front = image && IMG + last + 1 <= R::REACH_ROWS;
    const long long base = front ? 0 : IMG + a.row0, back = IMG + total;
    for (int i = 0; i < R::WORDS; ++i) {
        const int s = i < G::NR ? src[i < G::NR ? i : 0] : S3_SRC_NONE;
        const bool none = s == S3_SRC_NONE, img = !none && (s & S3_SRC_IMAGE);
        const long long row = img ? (front ? 0 : back) + (s & ~S3_SRC_IMAGE) : IMG + s;
        const unsigned off = none ? R::OFF_NONE : (unsigned)((row - base) * R::ROWB) + (unsigned)((i < a.n ? t0a : t0b) * R::TILEB);
        w[i] = i == R::BASE ? (unsigned)base : off - ((unsigned)i << R::ROW_SHIFT);
    }
}

// ---- passes of TILE slots ----
// A pass of pair slots (above) fills 60 of the kernel's 64 tiles, and the matrix cores compute the other 4 anyway.  A pass of tile slots is up to
// 64 CONSECUTIVE TILES of its list's pair sequence instead: it begins `o` tiles into its first pair (o even: a conv row pair's two rows alternate
// along the tile numbering, and the kernel pools tiles 2k and 2k + 1) and may end inside its last one; a pair cut between two passes is staged by
// both, each computes its own tiles of it.  The runs, the block and the SPAN rule are the pair-slot passes'; after an early close (a third run, SPAN)
// the next pass begins at a pair boundary, because runs do.  Both lists are packed this way.
//   full width (Skip3TGeom):  o = 0 .. 8, o + 64 tiles touch at most 8 pairs: 2 * 8 + 4 * 2 = 24 V3 rows (25 row slots of 5440 bytes: 133 KB of LDS)
//   windowed (Skip3TXGeom):   o = 0 .. 4, o + 64 tiles touch 11 pairs and at o = 4 twelve: 2 * 12 + 4 * 2 = 32 V3 rows, two more than the 32-word
//                             row table of the pair-slot passes has room for (Skip3Reach: NR < WORDS - 1), so these passes have a row
//                             table of ROW_WORDS = 64 words, one per lane (skip3t_row_words).  33 row slots of 3264 bytes: 105 KB of LDS.
//                             Holding a pass to the 11 pairs a 32-word table allows was counted first: the pass that begins at o = 4 then
//                             closes at 62 tiles, and the benchmark's windowed crops -- all of 8 pairs, 48 tiles -- need four passes for five
//                             crops, as with pair slots (8 + 2, 6 + 4, 4 + 6, 2 + 8), where 48 + 16 | 32 + 32 | 16 + 48 are three for four:
//                             7349 windowed passes instead of 6901 on 25600 crops (profiles/conv3_tile_slots.txt).
// The descriptor is skip3_describe's of the pairs the pass TOUCHES (SLOTS pair slots), its row words skip3_row_words' (full width) or
// skip3t_row_words' (windowed) of them, and word S3_TILES carries o and the tile count.
struct Skip3TGeom {
    static constexpr int PAIRS = Skip3Geom::PAIRS, RUNS = Skip3Geom::RUNS, HALO = Skip3Geom::HALO, SPAN = Skip3Geom::SPAN, BLOCK = Skip3Geom::BLOCK;
    static constexpr int TILES = Skip3Geom::TILES, TPP = 2 * TILES;         // tiles of a row that a pass computes (all 5); tiles per pair
    static constexpr int MB = 64;                                           // tile slots of a pass
    static constexpr int MAXP = (TPP - 2 + MB + TPP - 1) / TPP;             // pairs a pass can touch (8)
    static constexpr int SLOTS = MAXP;                                      // pair slots of the descriptor
    static constexpr int NR = SkipGeom::POOL * MAXP + 2 * HALO * RUNS;      // V3 rows a pass can stage (24)
    static constexpr int BLOCK_PASSES = (BLOCK * PAIRS * TPP + MB - 1) / MB + BLOCK + 1;   // full passes + passes closed by a third run + the last
    static constexpr int DESC = 16;
    static constexpr int ROW_WORDS = 32;                                    // words of a pass's row table: Skip3Reach's
    static_assert(MAXP == 8 && NR == 24 && S3X_DESC_OK(DESC, SLOTS), "2 + 60 + 2 tiles: 8 pairs, and the descriptor holds their slots");
    static_assert((long long)(SPAN + SLOTS) * SkipGeom::POOL * 10240 < (1ll << 31), "V3 byte distance inside a pass");
};
struct Skip3TXGeom {
    static constexpr int PAIRS = Skip3Geom::PAIRS, RUNS = Skip3Geom::RUNS, HALO = Skip3Geom::HALO, SPAN = Skip3Geom::SPAN, BLOCK = Skip3Geom::BLOCK;
    static constexpr int WT3 = Skip3XGeom::WT3, TILES = WT3, TPP = 2 * TILES;
    static constexpr int MB = 64;
    static constexpr int MAXP = (TPP - 2 + MB + TPP - 1) / TPP;             // pairs a pass can touch (12: 2 + 60 + 2 tiles)
    static constexpr int SLOTS = MAXP;
    static constexpr int NR = SkipGeom::POOL * MAXP + 2 * HALO * RUNS;      // V3 rows a pass can stage (32)
    static constexpr int ROW_WORDS = 64;                                    // words of a pass's row table
    static constexpr int BLOCK_PASSES = (BLOCK * PAIRS * TPP + MB - 1) / MB + BLOCK + 1;
    static constexpr int DESC = 32;
    static_assert(MAXP == 12 && NR == 32 && NR < ROW_WORDS - 1, "12 pairs, and the row table holds their rows and `none`");
    static_assert(S3X_DESC_OK(DESC, SLOTS), "the descriptor holds the slots");
    static_assert((long long)(SPAN + SLOTS) * SkipGeom::POOL * 10240 < (1ll << 31), "V3 byte distance inside a pass");
};
template <class G> struct Skip3Tiled { static constexpr bool value = false; static constexpr int ROW_WORDS = 32 /* Skip3Reach::WORDS */; };
template <> struct Skip3Tiled<Skip3TGeom> { static constexpr bool value = true; static constexpr int ROW_WORDS = Skip3TGeom::ROW_WORDS; };
template <> struct Skip3Tiled<Skip3TXGeom> { static constexpr bool value = true; static constexpr int ROW_WORDS = Skip3TXGeom::ROW_WORDS; };

// a pass of tile slots while it is filled: n tiles from `runs` runs, the first one entered o tiles into the pair gp0[0]; run r touches the pairs
// gp0[r] .. gp0[r] + len[r] - 1 (the first of run A from tile o on, the last of the pass's last run maybe not to its end)
struct Skip3TPass { int n, runs, o, gp0[Skip3Geom::RUNS], len[Skip3Geom::RUNS]; };

// the tiles a pass that begins o tiles into a pair and has touched `pairs` pairs of earlier runs can still take of a run it enters at tile `off`
template <class T>
TREXHIP_HD constexpr int skip3t_room(const Skip3TPass& p, const int off) {
    const int touched = p.runs ? p.len[0] : 0;                              // (a second run is the last: only run A is in front of the one entered)
    const int by_pairs = (T::MAXP - touched) * T::TPP - off, by_tiles = T::MB - p.n;
    return by_pairs < by_tiles ? by_pairs : by_tiles;
}
// the pairs gp .. gp + len - 1 of one crop, from tile `off` of the first on (off != 0: only into an empty pass), go into the pass being filled and
// the passes behind it; emit(index, pass) takes every pass that closes.  A pass closes when it has no room (64 tiles, or MAXP pairs), when a
// third run would begin, or when the next run lies more than SPAN pairs behind its first pair
template <class T, class E>
TREXHIP_HD constexpr void skip3t_add_run(Skip3TPass& p, int& passes, int gp, const int len, E&& emit) {
    int left = len * T::TPP, off = 0;
    while (left > 0) {
        if (p.runs && (skip3t_room<T>(p, off) <= 0 || p.runs == T::RUNS || gp - p.gp0[0] > T::SPAN)) { emit(passes, p); ++passes; p = Skip3TPass{}; }
        const int room = skip3t_room<T>(p, off), take = left < room ? left : room;
        const int touch = (off + take + T::TPP - 1) / T::TPP;
        if (p.runs == 0) { p.o = off; p.gp0[0] = gp; p.len[0] = touch; }    // (no index that is a variable: the pass stays in registers on the device)
        else { p.gp0[1] = gp; p.len[1] = touch; }
        ++p.runs; p.n += take; left -= take;
        off += take; gp += off / T::TPP; off %= T::TPP;
        // a run that goes on behind this pass does so in an empty one
        if (left > 0) { emit(passes, p); ++passes; p = Skip3TPass{}; }
    }
}
template <class E>
TREXHIP_HD constexpr void skip3t_flush(Skip3TPass& p, int& passes, E&& emit) {
    if (p.n) { emit(passes, p); ++passes; p = Skip3TPass{}; }
}
// the pairs a pass of tile slots touches, as a pass of pair slots: what skip3_describe and skip3_row_words take
TREXHIP_HD constexpr Skip3Pass skip3t_pairs(const Skip3TPass& p) {
    Skip3Pass r{};
    r.runs = p.runs; r.gp0[0] = p.gp0[0]; r.len[0] = p.len[0];
    r.gp0[1] = p.runs > 1 ? p.gp0[1] : 0; r.len[1] = p.runs > 1 ? p.len[1] : 0;
    r.n = r.len[0] + r.len[1];
    return r;
}
// descriptor word S3_TILES of a pass of tile slots: o | tiles << 8.  Tile slot t of the pass is tile (o + t) % TPP of pair slot (o + t) / TPP
enum : int { S3_TILES = 6, S3_O_MASK = 0xff, S3_COUNT_SHIFT = 8 };
template <class T>
TREXHIP_HD constexpr void skip3t_describe(const Skip3TPass& p, int (&d)[T::DESC], const int t0a = 0, const int t0b = 0) {
    skip3_describe<T>(skip3t_pairs(p), d, t0a, t0b);
    d[S3_TILES] = p.o | p.n << S3_COUNT_SHIFT;
}
// The row words of a pass of tile slots: skip3_row_words' of the pairs it touches, in a table of T::ROW_WORDS words -- entry i < NR the source of
// row slot 1 + i, the entries behind them none, the last one the row of the allocation the resource starts at
template <class T>
TREXHIP_HD constexpr void skip3t_row_words(const Skip3Pass& p /* skip3t_pairs of the pass */, const SkipRows own_a, const SkipRows own_b, const long long total,
                                           unsigned (&w)[T::ROW_WORDS], const int t0a = 0, const int t0b = 0) {
    using R = Skip3Reach;
    constexpr int IMG = SkipGeom::V3_ROWS, BASE = T::ROW_WORDS - 1;
    int src[T::NR] = {};
    skip3_row_sources<T>(p, own_a, own_b, src);
    const bool two = p.runs > 1;
    const Skip3Rows a = skip3_run_rows(p.gp0[0], p.len[0]);
    const Skip3Rows b = two ? skip3_run_rows(p.gp0[1], p.len[1]) : Skip3Rows{a.row0 + a.n, 0};
    const long long last = b.row0 + b.n - 1;
    bool image = false;
    for (int i = 0; i < T::NR; ++i) image = image || (src[i] != S3_SRC_NONE && (src[i] & S3_SRC_IMAGE));
    const bool front = image && IMG + last + 1 <= R::REACH_ROWS;
    const long long base = front ? 0 : IMG + a.row0, back = IMG + total;
    for (int i = 0; i < T::ROW_WORDS; ++i) {
        const int s = i < T::NR ? src[i < T::NR ? i : 0] : S3_SRC_NONE;
        const bool none = s == S3_SRC_NONE, img = !none && (s & S3_SRC_IMAGE);
        const long long row = img ? (front ? 0 : back) + (s & ~S3_SRC_IMAGE) : IMG + s;
        const unsigned off = none ? R::OFF_NONE : (unsigned)((row - base) * R::ROWB) + (unsigned)((i < a.n ? t0a : t0b) * R::TILEB);
        w[i] = i == BASE ? (unsigned)base : off - ((unsigned)i << R::ROW_SHIFT);
    }
}
// every pass of tile slots of a batch of `total` V3 rows reaches an image (skip3_direct_fits, with the pairs these passes touch)
TREXHIP_HD constexpr bool skip3t_direct_fits(const long long total) {
    using R = Skip3Reach;
    return total <= 2 * R::REACH_ROWS - 2 * SkipGeom::V3_ROWS - ((Skip3TXGeom::SPAN + Skip3TXGeom::SLOTS) * SkipGeom::POOL + 2 * Skip3TXGeom::HALO) - 1;
}
static_assert(Skip3TGeom::NR < Skip3TGeom::ROW_WORDS - 1 && Skip3TGeom::ROW_WORDS == Skip3Reach::WORDS, "the row table holds a pass's rows and `none`");

// (the words of Net::d_skip that the kernels of the listed conv3 and fc1 write and read: cnn_skip_words.h)

// fc1's split-K plane s is row pair q = s of every crop (FC1_KSPLIT planes of 10 x 128 inputs), and a crop's row of an MFMA tile depends on
// that crop's activations and the weights alone: the partial sum of a pair that holds the empty crop's bits is, bit for bit, plane q of fc1 run on
// the empty crop's act3 (Net::fc1e, made once per loaded network).  The ONE rule that says which (crop, plane) the listed fc1 computes and the
// head reads from memory -- the list kernel and the head call this function: every pair where the empty crop left the fp16 range (`all`: the
// word SK_EMPTY_RANGE), else the pairs conv3's rule lists.  It does not depend on the form of conv3 that ran: behind the dense one an unlisted
// pair holds the empty crop's bits just the same.
static_assert(Skip3Geom::PAIRS == FC1_KSPLIT, "plane s of the split-K fc1 is row pair s");
TREXHIP_HD constexpr bool skip3_fc1_listed(const bool all, const SkipBand b, const int q) {
    if (all) return true;
    const SkipPairs r = skip3_pairs(b);
    return q >= r.lo && q <= r.hi;
}

// listed passes against the dense kernel's: the listed form runs when  listed * FACTOR_NUM < dense * FACTOR_DEN.  The factor is what a listed
// pass costs in dense passes, measured on the benchmark's crops under a kernel trace (profiles/v3_direct_rows.txt): 3542 us for 31393 listed
// passes = 112.8 ns against 4539 us for the dense kernel's 40000 = 113.5 ns: 0.994, and 1.004 against the parent build's dense kernel on the same
// box -- 1.00.  (1.010 while the listed form read its background rows from a copy in V3, profiles/conv3_listed_pairs.txt.)  Noise crops (every
// pair listed: 1.067 times the dense passes) stay dense, the benchmark's crops (0.785) are listed.  What the list kernels cost is the same either
// way; k_v3_fill's copy, which only the dense form needs now, is left out of the choice: it matters where the two forms are within a few percent
static constexpr int SKIP3_FACTOR_NUM = 100, SKIP3_FACTOR_DEN = 100;
TREXHIP_HD constexpr bool skip3_use_list(const long long listed, const long long dense) {
    return listed * SKIP3_FACTOR_NUM < dense * SKIP3_FACTOR_DEN;
}

}  // namespace trexhip
