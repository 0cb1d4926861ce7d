// cnn_skipx.h -- the skipping rule of cnn_skip.h in x: which conv2 tiles (Winograd F(4,5) tiles of 4 output columns) of an 80 x 80 identity crop
// can differ from the all-zero crop's, the window of WT tiles a crop's blob fits into, and the packing of a crop's needed V3 rows into the
// windowed passes of k_conv12_rs<W12XGeom> (cnn_fused12rs.h).  Pure constexpr, no device code and no HIP: the device kernels
// (cnn_skip_kernels.h, cnn_fused12rs.h) and tests/cpp/test_cnn_skipx.cpp read the same functions.
//
// cnn_skip.h looks at rows only.  A blob is narrow as well: a tile whose whole 8-pixel V2 input window equals the empty crop's -- in every row
// the tile's output row reads -- has the empty crop's bits, for the reason cnn_skip.h gives for rows.  A windowed pass computes WT of a row's 10
// tiles for WR conv2 rows of ONE crop (WT x WR = 64 M-slots, none idle) and takes the pooled activations outside the window from an image of
// the empty crop's (Net::act2e, made by the run that makes Net::v3e).
#pragma once
#include "cnn_skip.h"

namespace trexhip {

struct SkipXGeom {
    static constexpr int TILE = 4;                                          // conv2 output columns per F(4,5) tile
    static constexpr int TILES = W2bGeom::S / TILE;                         // 10 per row
    static constexpr int WT = 8, WR = 8;                                    // the window: tiles x conv2 rows
    static constexpr int RPP = WR / SkipGeom::POOL;                         // V3 rows per windowed pass
    static constexpr int NR = WR + W2bGeom::KH - 1;                         // V2 rows a windowed pass reads
    static constexpr int CHUNK = WR;                                        // V2 rows the producers make per three stages
    // tile t reads the V2 columns TILE t - KH / 2 .. TILE t + TILE - 1 + KH / 2, V2 column c the crop columns skip_layer_lo(c) .. skip_layer_hi(c)
    static constexpr int V2_LO0 = -(W2bGeom::KH / 2), V2_HI0 = TILE - 1 + W2bGeom::KH / 2;
    static constexpr int STEP = TILE * SkipGeom::POOL, LO0 = skip_layer_lo(V2_LO0), HI0 = skip_layer_hi(V2_HI0);
    static_assert(STEP == 8 && LO0 == -6 && HI0 == 13, "tile t reads crop columns 8 t - 6 .. 8 t + 13");
    static_assert(WT * WR == 64 && WT <= TILES && RPP * SkipGeom::POOL == WR, "one MFMA M block, whole pooled rows");
};

// the conv2 tiles of a crop that can differ from the empty crop's, from its first and last non-zero COLUMN (SkipBand's y0, y1 read as x0, x1); none: lo > hi
struct SkipTiles { int lo, hi; };
TREXHIP_HD constexpr SkipTiles skipx_tiles(const SkipBand b) {
    using X = SkipXGeom;
    if (b.y0 > b.y1) return {1, 0};
    // STEP t + HI0 >= x0  and  STEP t + LO0 <= x1
    const int lo = b.y0 <= X::HI0 ? 0 : (b.y0 - X::HI0 + X::STEP - 1) / X::STEP;
    const int hi = (b.y1 - X::LO0) / X::STEP;
    return {lo, hi < X::TILES - 1 ? hi : X::TILES - 1};
}

// the window [t0, t0 + WT) of a crop; -1: it has none (wider than WT tiles, or the empty crop's image is not to be used).  A crop without a
// blob needs no pass at all; its window is 0
TREXHIP_HD constexpr int skipx_window(const SkipBand cols, const bool empty_out_of_range) {
    using X = SkipXGeom;
    if (empty_out_of_range) return -1;
    const SkipTiles t = skipx_tiles(cols);
    if (t.lo > t.hi) return 0;
    if (t.hi - t.lo + 1 > X::WT) return -1;
    return t.lo < X::TILES - X::WT ? t.lo : X::TILES - X::WT;
}

// a windowed pass as one list entry: crop, first V3 row of the crop, rows (1 .. RPP), t0
struct SkipXPass { int crop, r0, rows, t0; };
static constexpr int SKIPX_MAX_CROPS = 1 << 22;
TREXHIP_HD constexpr int skipx_pack(const SkipXPass p) { return p.crop << 9 | p.r0 << 4 | (p.rows - 1) << 2 | p.t0; }
TREXHIP_HD constexpr SkipXPass skipx_unpack(const int e) { return {e >> 9, (e >> 4) & 31, ((e >> 2) & 3) + 1, e & 3}; }
static_assert(SkipXGeom::RPP <= 4 && SkipXGeom::TILES - SkipXGeom::WT <= 3 && SkipGeom::V3_ROWS <= 32, "the fields of an entry");

// the windowed passes of a crop: its needed rows (skip_rows) as one run, cut into passes of RPP rows from its first row on; the last may be short
TREXHIP_HD constexpr int skipx_passes(const SkipRows need) {
    return need.lo > need.hi ? 0 : (need.hi - need.lo + 1 + SkipXGeom::RPP - 1) / SkipXGeom::RPP;
}
TREXHIP_HD constexpr SkipXPass skipx_pass(const int crop, const SkipRows need, const int t0, const int k /* 0 .. skipx_passes - 1 */) {
    const int r0 = need.lo + k * SkipXGeom::RPP, left = need.hi - r0 + 1;
    return {crop, r0, left < SkipXGeom::RPP ? left : SkipXGeom::RPP, t0};
}

// must full-width pass p be computed, where the crops with a window take windowed passes?  Only for a row that a crop WITHOUT a window needs.
// band(crop), win(crop): the crop's row band and its window (-1: none)
template <class B, class W>
TREXHIP_HD constexpr bool skipx_full_needed(const int p, const int total_pairs, const B& band, const W& win) {
    using G = SkipGeom;
    for (int gp = p * G::RPP; gp < (p + 1) * G::RPP && gp < total_pairs; ++gp) {
        const int crop = gp / G::V3_ROWS, r = gp - crop * G::V3_ROWS;
        if (win(crop) >= 0) continue;
        const SkipRows need = skip_rows(band(crop));
        if (r >= need.lo && r <= need.hi) return true;
    }
    return false;
}

// The V2 rows (conv1's pooled rows, 0 .. V2_ROWS - 1) of a crop that have a non-zero crop row under them, from its first and last non-zero
// ROW: V2 row y reads the crop rows skip_layer_lo(y) .. skip_layer_hi(y) = 2 y - 2 .. 2 y + 3.  None: lo > hi.  Every other V2 row of the crop is
// the BACKGROUND row: conv1's accumulator is exactly 0 for each of its pixels (background is 0, and so is the padding around the crop), each
// pixel is relu(0 * inv_scale1 + bias) -- the same in every crop and at every y.  The windowed instance does not make such rows: its consumers
// read them from a row slot made once per workgroup and first tile t0 (conv2's zero padding at tiles 0 and 9 is all that makes it depend on t0)
struct SkipV2 { int lo, hi; };
static constexpr SkipV2 SKIPX_V2_ALL{0, SkipGeom::V2_ROWS - 1};
TREXHIP_HD constexpr SkipV2 skipx_v2_rows(const SkipBand b) {
    using G = SkipGeom;
    if (b.y0 > b.y1) return {1, 0};
    // skip_layer_hi(y) >= y0  and  skip_layer_lo(y) <= y1
    constexpr int HI0 = skip_layer_hi(0), LO0 = skip_layer_lo(0);
    const int lo = b.y0 <= HI0 ? 0 : (b.y0 - HI0 + G::POOL - 1) / G::POOL;
    const int hi = (b.y1 - LO0) / G::POOL;
    return {lo, hi < G::V2_ROWS - 1 ? hi : G::V2_ROWS - 1};
}
// a crop's range as the word k_pass_list writes beside every windowed list entry (Net::skipx_rows): both roles of the kernel read it as a scalar,
// one round ahead, like the entry itself
TREXHIP_HD constexpr int skipx_v2_pack(const SkipV2 v) { return v.lo | v.hi << 8; }
TREXHIP_HD constexpr SkipV2 skipx_v2_unpack(const int w) { return {w & 0xff, (w >> 8) & 0xff}; }

// The stages (s_barrier) of one round of k_conv12_rs, either instance: three for the taps beside the first chunk of the V2 rows the producers
// make for the next pass, three more per further chunk.  Called by rs_round alone.
TREXHIP_HD constexpr int rs_round_chunks(const int made_rows, const int chunk) { return made_rows <= chunk ? 1 : (made_rows + chunk - 1) / chunk; }
TREXHIP_HD constexpr int rs_round_stages(const int made_rows, const int chunk) { return 3 * rs_round_chunks(made_rows, chunk); }

// the V2 rows [qmin, qmin + nrows) of the batch that the V3 rows gp0 .. gpl (of one crop, or of the aligned pass) read: two halo rows either
// side where the crop has them
struct SkipXV2 { int qmin, nrows; };
TREXHIP_HD constexpr SkipXV2 rs_v2_rows(const int gp0, const int gpl) {
    constexpr int S = W2bGeom::S;
    const int y0 = (2 * gp0) % S, yl = (2 * gpl) % S + 1;
    const int qmin = 2 * gp0 - (y0 >= 2 ? 2 : 0);
    return {qmin, 2 * gpl + 1 + (yl + 2 <= S - 1 ? 2 : 0) - qmin + 1};
}
// the new rows [lo, hi) of a round: the next pass's rows, less those the ring holds already where it follows the current one
TREXHIP_HD constexpr SkipXV2 rs_new_rows(const bool follows, const int res_hi, const int gp0n, const int gpln) {
    const SkipXV2 v = rs_v2_rows(gp0n, gpln);
    const int lo = (follows && res_hi > v.qmin) ? res_hi : v.qmin;
    return {lo, v.qmin + v.nrows - lo};
}
// One round of k_conv12_rs, as BOTH roles take it from this one function on the same data: the new rows [lo, hi) of the next pass (rs_new_rows;
// the ring counts as holding them from then on), the rows [clo, chi) of them the producers make -- `clip`: those inside the range `v2` of the
// pass's crop (the windowed instance, whose pass holds one crop: the others are background rows, which nobody makes and the consumers read from
// the background slot); otherwise all of them -- and the chunks of the round, by the rows MADE: the roles cannot execute different numbers
// of barriers.  A first pass: follows = false.
struct RsRound { int lo, hi, clo, chi, chunks; };
TREXHIP_HD constexpr RsRound rs_round(const bool follows, const int res_hi, const int gp0n, const int gpln, const bool clip, const SkipV2 v2, const int chunk) {
    constexpr int S = W2bGeom::S;
    const SkipXV2 nw = rs_new_rows(follows, res_hi, gp0n, gpln);
    const int lo = nw.qmin, hi = nw.qmin + nw.nrows;
    int clo = lo, chi = hi;
    if (clip) {
        const int base = (gp0n / (S / 2)) * S;                              // the crop's first V2 row of the batch
        clo = lo > base + v2.lo ? lo : base + v2.lo;
        chi = hi < base + v2.hi + 1 ? hi : base + v2.hi + 1;
        if (chi < clo) chi = clo;
    }
    return {lo, hi, clo, chi, rs_round_chunks(chi - clo, chunk)};
}
// no round: the last pass of a workgroup has no next one
static constexpr RsRound RS_ROUND_NONE{0, 0, 0, 0, 1};

}  // namespace trexhip
