// Prints what the column rule of conv3, its windows and the packing of the windowed listed passes (trex_amd/csrc/cnn_skip3.h) say;
// tests/test_cnn_skip3x.py holds them to a brute-force propagation and to hand-derived numbers.
//   tiles                          "x0 x1 lo hi" for no non-zero column (x0 = 80, x1 = -1) and for every 0 <= x0 <= x1 < 80
//   window x0 x1 out_of_range      the window's first tile, -1: none
//   windows                        "x0 x1 t0" for every 0 <= x0 <= x1 < 80, the empty crop in range
//   pack total first y0:y1:x0:x1 ...   the crops first, first + 1, ... of a batch of `total` crops, one block of the list kernels: the windowed passes
//                                  of those that have a window, as the device makes them (skip3_add_run, skip3_describe and skip3_row_words on
//                                  Skip3XGeom), every word decoded:
//                                    "pass idx pairs runs rows base"             base: the row of V3's allocation its resource starts at
//                                    "slot s pair q t0 ldsrow"                   pair: crop * 10 + q of the batch; an idle slot: pair -1
//                                    "row i allocrow byte"                       LDS row slot 1 + i <- that byte of that row of the allocation; none: -1 -1
//   plan geom n                    "skip3=<0|1> v3_direct=<0|1> skip3x=<0|1>" of the 80 x 80 one-channel FP16X3 plan on 256 CUs
#include "../../trex_amd/csrc/cnn_plan.h"
#include "../../trex_amd/csrc/cnn_skip3.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace trexhip;

static_assert(skip3_tiles(SKIP_BAND_NONE).lo > skip3_tiles(SKIP_BAND_NONE).hi && skip3_window(SKIP_BAND_NONE, false) == -1, "usable in constant expressions");
static_assert(skip3_window({40, 40}, false) == 1 && skip3_window({40, 40}, true) == -1 && skip3_window({0, 79}, false) == -1, "a pixel, no image, a full crop");
static_assert(Skip3XGeom::WT3 == 3 && Skip3XGeom::SLOTS * 2 * Skip3XGeom::WT3 == 60 && Skip3XGeom::NR == 28 && Skip3XGeom::DESC == 32, "the windowed pass");

int main(int argc, char** argv) {
    using X = Skip3XGeom;
    using R = Skip3Reach;
    if (argc == 2 && !std::strcmp(argv[1], "tiles")) {
        const Skip3Tiles none = skip3_tiles(SKIP_BAND_NONE);
        std::printf("%d %d %d %d\n", SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1, none.lo, none.hi);
        for (int x0 = 0; x0 < 80; ++x0)
            for (int x1 = x0; x1 < 80; ++x1) {
                const Skip3Tiles t = skip3_tiles({x0, x1});
                std::printf("%d %d %d %d\n", x0, x1, t.lo, t.hi);
            }
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "window")) {
        std::printf("%d\n", skip3_window({std::atoi(argv[2]), std::atoi(argv[3])}, std::atoi(argv[4]) != 0));
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "windows")) {
        for (int x0 = 0; x0 < 80; ++x0)
            for (int x1 = x0; x1 < 80; ++x1) std::printf("%d %d %d\n", x0, x1, skip3_window({x0, x1}, false));
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "pack")) {
        const long long total = std::atoll(argv[2]) * SkipGeom::V3_ROWS;
        const int first = std::atoi(argv[3]);
        std::vector<SkipBand> bands, cols;
        for (int i = 4; i < argc; ++i) {
            SkipBand b, c;
            if (std::sscanf(argv[i], "%d:%d:%d:%d", &b.y0, &b.y1, &c.y0, &c.y1) != 4) { std::fprintf(stderr, "bad crop: %s\n", argv[i]); return 2; }
            bands.push_back(b);
            cols.push_back(c);
        }
        if ((int)bands.size() > X::BLOCK) { std::fprintf(stderr, "one block is %d crops\n", X::BLOCK); return 2; }
        auto emit = [&](const int idx, const Skip3Pass& p) {
            const int ca = p.gp0[0] / X::PAIRS - first, cb = (p.runs > 1 ? p.gp0[1] : p.gp0[0]) / X::PAIRS - first;
            const int t0a = skip3_window(cols.at((size_t)ca), false), t0b = skip3_window(cols.at((size_t)cb), false);
            int d[X::DESC];
            unsigned w[R::WORDS];
            skip3_describe<X>(p, d, t0a, t0b);
            skip3_row_words<X>(p, skip_rows(bands.at((size_t)ca)), skip_rows(bands.at((size_t)cb)), total, w, t0a, t0b);
            std::printf("pass %d %d %d %d %u\n", idx, p.n, p.runs, d[S3_ROWS], w[R::BASE]);
            for (int s = 0; s < X::SLOTS; ++s) {
                const unsigned e = (unsigned)d[S3_SLOT + s];
                const bool idle = (e >> 16) == (unsigned)S3_IDLE;
                std::printf("slot %d %d %d %d %d\n", s, idle ? -1 : d[S3_GP0] + (int)(e >> 16), (int)((e >> 8) & S3_Q_MASK), (int)((e >> S3_T0_SHIFT) & S3_T0_MASK), (int)(e & 0xff));
            }
            for (int i = 0; i < R::WORDS - 1; ++i) {
                const unsigned off = w[i] + ((unsigned)i << R::ROW_SHIFT);
                if (off >= R::NUM_RECORDS) { std::printf("row %d -1 -1\n", i); continue; }
                if (off >= R::REACH) { std::fprintf(stderr, "row %d: offset %u out of reach\n", i, off); std::exit(3); }
                std::printf("row %d %lld %u\n", i, (long long)w[R::BASE] + off / R::ROWB, off % R::ROWB);
            }
        };
        Skip3Pass p{};
        int passes = 0;
        for (size_t c = 0; c < bands.size(); ++c) {
            const SkipPairs r = skip3_pairs(bands[c]);
            if (r.lo <= r.hi && skip3_window(cols[c], false) >= 0) skip3_add_run<X>(p, passes, (first + (int)c) * X::PAIRS + r.lo, r.hi - r.lo + 1, emit);
        }
        skip3_flush(p, passes, emit);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, (int)std::atoll(argv[2]), std::atoi(argv[3]), 256);
        std::printf("skip3=%d v3_direct=%d skip3x=%d\n", (int)p.skip3, (int)p.v3_direct, (int)p.skip3x);
        return 0;
    }
    std::fprintf(stderr, "usage: tiles | window x0 x1 range | windows | pack total first y0:y1:x0:x1 ... | plan geom n\n");
    return 2;
}
