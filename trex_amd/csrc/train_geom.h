// train_geom.h -- the geometry of the training chain at any individual_image_size (train_any.hip): the sizes of every level, the
// tiles and grids of the three roles of a convolution (forward, data gradient, weight gradient), fc1's positions and the buffer sizes, as one
// pure function of (W, H, CH).  (At 80x80 the planes and fc1's positions are read from it; the convolutions there are train.hip's own.)  No device code and no HIP: train.hip sizes its buffers and train_any.hip its launches from it, and
// tests/cpp/test_train_geom.cpp holds it to hand-derived numbers.
#pragma once
#include <stddef.h>
#include "cnn_geom.h"

namespace trexhip {

constexpr int TA_C1T = 16;                   // conv1 forward: a workgroup's tile is 16 x 16 pixels, one per thread
constexpr int TA_WG1_ROWS = 8, TA_WG1_COLS = 64;   // conv1 weight gradient: a workgroup's band of rows and strip of columns
constexpr int TA_HID = 100;                  // fc1 outputs

// One role's 2-D tiling of a layer: the k_tany_conv tiles are 64 pool windows (cnn_geom.h: any_tiles) over the ceil(h / 2) x ceil(w / 2)
// windows of a plane of h x w pixels -- ceil, not floor: the odd last row and column lie in no pool window, but they are convolution outputs
// (and gradients) like every other pixel
struct TrainAnyLayer {
    int C, CI;                               // output / input channels of the block's convolution
    int h, w;                                // its output plane z [n][h][w][C]; the pooled a and da are [n][h / 2][w / 2][C]
    AnyTiles tiles;                          // forward and data gradient (blocks 2, 3): both write a plane of h x w pixels
    int wg_types, wg_max_shares;             // weight gradient (blocks 2, 3): grid (types, shares)
};

struct TrainAnyGeom {
    int W, H, CH;
    int taps;                                // the convolutions are taps x taps with a halo of taps / 2: 5 (the identity networks) or 3 (the category network)
    TrainAnyLayer L[3];
    int h3, w3, P;                           // fc1: positions of the last pooled plane, P = (H / 8)(W / 8) by successive floors; the partial planes
                                             // of fc1 are the positions in row-major order (y * w3 + x), summed 0, 1, .. P - 1
    int c1_tx, c1_tiles;                     // conv1 forward: tiles per row / per crop
    int wg1_tx, wg1_tiles;                   // conv1 weight gradient: strips per band / workgroups per crop

    // the weight gradient of block i (1, 2) walks the n * h rows of the batch in `shares` contiguous runs of `per` rows: a function of the size
    // and n alone, so the partials and their order are the same in every run
    int wg_per(const int i, const int n) const {
        const long long rows = (long long)n * L[i].h;
        const long long s = rows < L[i].wg_max_shares ? rows : L[i].wg_max_shares;
        return (int)((rows + s - 1) / s);
    }
    int wg_shares(const int i, const int n) const {
        const long long rows = (long long)n * L[i].h;
        const int per = wg_per(i, n);
        return (int)((rows + per - 1) / per);
    }

    // buffer sizes in floats at a batch of n
    size_t x_floats(const size_t n) const { return n * H * W * CH; }
    size_t z_floats(const int i, const size_t n) const { return n * L[i].h * L[i].w * L[i].C; }
    size_t a_floats(const int i, const size_t n) const { return n * (L[i].h / 2) * (L[i].w / 2) * L[i].C; }
    size_t hpart_floats(const size_t n) const { return n * P * TA_HID; }
    size_t part_floats() const {
        const size_t t2 = (size_t)taps * taps;
        const size_t p1 = (size_t)L[1].wg_max_shares * t2 * L[1].CI * L[1].C, p2 = (size_t)L[2].wg_max_shares * t2 * L[2].CI * L[2].C;
        return p1 > p2 ? p1 : p2;
    }
    size_t part1_floats(const size_t n) const { return n * wg1_tiles * CH * taps * taps * 16; }
    size_t fc1_weight_floats() const { return (size_t)P * 128 * TA_HID; }
};

inline TrainAnyGeom train_any_geom(const int W, const int H, const int CH, const int taps = 5) {
    TrainAnyGeom g{};
    g.W = W; g.H = H; g.CH = CH; g.taps = taps;
    const int C[3] = {16, 64, 128};
    int h = H, w = W;
    // successive floors: every level halves the one above it and has an odd edge of its own (21 -> 10 -> 5 -> 2, 13 -> 6 -> 3 -> 1)
    for (int i = 0; i < 3; ++i) {
        g.L[i].C = C[i]; g.L[i].CI = i ? C[i - 1] : CH;
        g.L[i].h = h; g.L[i].w = w;
        g.L[i].tiles = any_tiles((h + 1) / 2, (w + 1) / 2);
        h /= 2; w /= 2;
    }
    g.h3 = h; g.w3 = w; g.P = h * w;
    // weight gradients: a workgroup type is a kernel row x a 32-wide slice of the input channels (conv2: 16 channels x 2 taps per slice), so
    // taps and 2 taps types: 5 and 10 at 5 taps, 3 and 6 at 3; the shares keep the 5-tap grid near two workgroups per CU of the 256
    g.L[0].wg_types = 0; g.L[0].wg_max_shares = 0;
    g.L[1].wg_types = taps; g.L[1].wg_max_shares = 96;
    g.L[2].wg_types = 2 * taps; g.L[2].wg_max_shares = 48;
    g.c1_tx = (W + TA_C1T - 1) / TA_C1T;
    g.c1_tiles = ((H + TA_C1T - 1) / TA_C1T) * g.c1_tx;
    g.wg1_tx = (W + TA_WG1_COLS - 1) / TA_WG1_COLS;
    g.wg1_tiles = ((H + TA_WG1_ROWS - 1) / TA_WG1_ROWS) * g.wg1_tx;
    return g;
}

}  // namespace trexhip
