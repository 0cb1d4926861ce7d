// cnn_skip.h -- which rows of conv2's pooled output (the V3 image) depend on which rows of an 80 x 80 identity crop, and so which passes of the
// role-split conv1+conv2 kernel (cnn_fused12rs.h) a batch needs at all.  Pure constexpr, no device code and no HIP: the device kernels
// (cnn_skip_kernels.h) and tests/cpp/test_cnn_skip.cpp read the same functions.
//
// A crop is a blob painted into a box that is centre-padded with zeros: most of its rows are background.  A V3 row whose whole band of crop
// rows is zero equals, bit for bit, the same row of the V3 image of an all-zero crop (every window of it is zero across the full width, the
// padding above and below the crop is the same, and the kernel's arithmetic per output element does not depend on the pass, tile or lane it
// lands in), so that row is copied from an image made once per loaded network instead of being computed.
#pragma once
#include "cnn_geom.h"

#if defined(__HIP__)
#define TREXHIP_HD __host__ __device__
#else
#define TREXHIP_HD
#endif

namespace trexhip {

// one layer (W2bGeom::KH x KH 'same' convolution, POOL x POOL max-pool, the constants k_conv12_rs's row arithmetic uses; both layers are this):
// pooled output row r reads the input rows [POOL r - KH / 2, POOL r + POOL - 1 + KH / 2]
static constexpr int SKIP_KH = W2bGeom::KH, SKIP_POOL = W2bGeom::POOL;
TREXHIP_HD constexpr int skip_layer_lo(const int r) { return SKIP_POOL * r - SKIP_KH / 2; }
TREXHIP_HD constexpr int skip_layer_hi(const int r) { return SKIP_POOL * r + SKIP_POOL - 1 + SKIP_KH / 2; }

struct SkipGeom {
    static constexpr int POOL = SKIP_POOL;
    static constexpr int V2_ROWS = W2bGeom::S;                              // conv1's pooled rows per crop (40)
    static constexpr int CROP_ROWS = V2_ROWS * POOL;                        // 80
    static constexpr int V3_ROWS = V2_ROWS / POOL;                          // conv2's pooled rows per crop (20): the `pairs` of the kernels
    static constexpr int RPP = W2bGeom::RPP;                                // V3 rows per pass
    // two layers: V3 row gp reads the crop rows [STEP gp + LO0, STEP gp + HI0] (clipped to the crop; rows outside it are padding either way)
    static constexpr int STEP = POOL * POOL, LO0 = skip_layer_lo(skip_layer_lo(0)), HI0 = skip_layer_hi(skip_layer_hi(0));
    static_assert(STEP == 4 && LO0 == -6 && HI0 == 9, "V3 row gp reads crop rows 4 gp - 6 .. 4 gp + 9");
    static_assert(skip_layer_lo(skip_layer_lo(3)) == STEP * 3 + LO0 && skip_layer_hi(skip_layer_hi(3)) == STEP * 3 + HI0, "the band is affine in the row");
};

// first and last non-zero row of a crop; none: y0 > y1
struct SkipBand { int y0, y1; };
static constexpr SkipBand SKIP_BAND_NONE{SkipGeom::CROP_ROWS, -1};
// the V3 rows of the crop that must be computed; none: lo > hi
struct SkipRows { int lo, hi; };

TREXHIP_HD constexpr SkipRows skip_rows(const SkipBand b) {
    using G = SkipGeom;
    if (b.y0 > b.y1) return {1, 0};
    // STEP gp + HI0 >= y0  and  STEP gp + LO0 <= y1
    const int lo = b.y0 <= G::HI0 ? 0 : (b.y0 - G::HI0 + G::STEP - 1) / G::STEP;
    const int hi = (b.y1 - G::LO0) / G::STEP;                               // (y1 - LO0 >= 0)
    return {lo, hi < G::V3_ROWS - 1 ? hi : G::V3_ROWS - 1};
}

// must global pass p -- the V3 rows RPP p .. RPP p + RPP - 1 of the batch, as many of them as exist; they may belong to two crops -- be computed?
// band(crop) gives the crop's SkipBand
template <class B>
TREXHIP_HD constexpr bool skip_pass_needed(const int p, const int total_pairs, const B& band) {
    using G = SkipGeom;
    for (int gp = p * G::RPP; gp < (p + 1) * G::RPP && gp < total_pairs; ++gp) {
        const int crop = gp / G::V3_ROWS, r = gp - crop * G::V3_ROWS;
        const SkipRows need = skip_rows(band(crop));
        if (r >= need.lo && r <= need.hi) return true;
    }
    return false;
}

}  // namespace trexhip
