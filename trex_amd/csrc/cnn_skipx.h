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

// The stages (s_barrier) of one round of k_conv12_rs, either instance: three for the taps beside the first chunk of the next pass's new V2 rows,
// three more per further chunk.  BOTH roles call this with the same count of new rows: they cannot execute different numbers of barriers.
TREXHIP_HD constexpr int rs_round_chunks(const int new_rows, const int chunk) { return new_rows <= chunk ? 1 : (new_rows + chunk - 1) / chunk; }
TREXHIP_HD constexpr int rs_round_stages(const int new_rows, const int chunk) { return 3 * rs_round_chunks(new_rows, chunk); }

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

}  // namespace trexhip
