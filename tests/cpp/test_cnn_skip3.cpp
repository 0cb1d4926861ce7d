// Prints what the row-pair rule and the pass packing of the listed conv3 (trex_amd/csrc/cnn_skip3.h) say; tests/test_cnn_skip3.py holds them to a
// brute-force propagation of dependence and to hand-derived pass counts.
//   pairs                        "y0 y1 lo hi" for no non-zero row (y0 = 80, y1 = -1) and for every 0 <= y0 <= y1 < 80
//   window q                     "lo hi": the crop rows row pair q reads, composed from the three layers' windows (not clipped to the crop)
//   pack q0:len q0:len ...       one crop per argument, its listed pairs q0 .. q0 + len - 1 (len 0: none); one line per pass: the DESC words
//   plan geom n                  "chain=<0 for role split> skip=<0|1> skip3=<0|1> grid=<list kernels> fill=<k_act3_fill>" on 256 CUs
//   use listed dense             "1" when the listed form runs for these pass counts, else "0"
#include "../../trex_amd/csrc/cnn_plan.h"
#include "../../trex_amd/csrc/cnn_skip3.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace trexhip;

static_assert(skip3_pairs(SKIP_BAND_NONE).lo > skip3_pairs(SKIP_BAND_NONE).hi, "usable in constant expressions");
static_assert(skip3_pairs({0, 79}).lo == 0 && skip3_pairs({0, 79}).hi == Skip3Geom::PAIRS - 1, "a full crop lists every pair");

int main(int argc, char** argv) {
    using G = Skip3Geom;
    if (argc >= 2 && !std::strcmp(argv[1], "pairs")) {
        const SkipPairs none = skip3_pairs(SKIP_BAND_NONE);
        std::printf("%d %d %d %d\n", SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1, none.lo, none.hi);
        for (int y0 = 0; y0 < SkipGeom::CROP_ROWS; ++y0)
            for (int y1 = y0; y1 < SkipGeom::CROP_ROWS; ++y1) {
                const SkipPairs r = skip3_pairs({y0, y1});
                std::printf("%d %d %d %d\n", y0, y1, r.lo, r.hi);
            }
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "window")) {
        const int q = std::atoi(argv[2]);
        std::printf("%d %d\n", skip_layer_lo(skip_layer_lo(skip_layer_lo(q))), skip_layer_hi(skip_layer_hi(skip_layer_hi(q))));
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "pack")) {
        Skip3Pass p{};
        int passes = 0;
        auto emit = [](const int idx, const Skip3Pass& q) {
            int d[G::DESC];
            skip3_describe(q, d);
            std::printf("%d:", idx);
            for (int i = 0; i < G::DESC; ++i) std::printf(" %d", d[i]);
            std::printf("\n");
        };
        for (int i = 2; i < argc; ++i) {
            int q0, len;
            if (std::sscanf(argv[i], "%d:%d", &q0, &len) != 2 || q0 < 0 || len < 0 || q0 + len > G::PAIRS) { std::fprintf(stderr, "bad run: %s\n", argv[i]); return 2; }
            skip3_add_run(p, passes, (i - 2) * G::PAIRS + q0, len, emit);
        }
        skip3_flush(p, passes, emit);
        std::printf("passes %d\n", passes);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, (int)std::atoll(argv[2]), std::atoi(argv[3]), 256);
        std::printf("chain=%d skip=%d skip3=%d grid=%d fill=%d\n", (int)p.chain, (int)p.skip, (int)p.skip3, p.skip3_grid, p.act3_fill.grid);
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "use")) {
        std::printf("%d\n", (int)skip3_use_list(std::atoll(argv[2]), std::atoll(argv[3])));
        return 0;
    }
    std::fprintf(stderr, "usage: pairs | window q | pack q0:len ... | plan geom n | use listed dense\n");
    return 2;
}
