// Prints what the row-skipping rule of the role-split conv1+conv2 kernel (trex_amd/csrc/cnn_skip.h) says; tests/test_cnn_skip.py holds it to a
// brute-force propagation of dependence written on its own.
//   rows                         "y0 y1 lo hi" for no non-zero row (y0 = 80, y1 = -1) and for every 0 <= y0 <= y1 < 80
//   passes y0:y1 y0:y1 ...       one crop per argument: a line of 0 / 1, one character per pass of the batch
//   plan geom n                  "chain=<0 for role split> skip=<0|1>" of the 80 x 80 one-channel FP16X3 plan on 256 CUs
#include "../../trex_amd/csrc/cnn_plan.h"
#include "../../trex_amd/csrc/cnn_skip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace trexhip;

static_assert(skip_rows(SKIP_BAND_NONE).lo > skip_rows(SKIP_BAND_NONE).hi, "usable in constant expressions");

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "rows")) {
        const SkipRows none = skip_rows(SKIP_BAND_NONE);
        std::printf("%d %d %d %d\n", SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1, none.lo, none.hi);
        for (int y0 = 0; y0 < SkipGeom::CROP_ROWS; ++y0)
            for (int y1 = y0; y1 < SkipGeom::CROP_ROWS; ++y1) {
                const SkipRows r = skip_rows({y0, y1});
                std::printf("%d %d %d %d\n", y0, y1, r.lo, r.hi);
            }
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "passes")) {
        std::vector<SkipBand> bands;
        for (int i = 2; i < argc; ++i) {
            SkipBand b;
            if (std::sscanf(argv[i], "%d:%d", &b.y0, &b.y1) != 2) { std::fprintf(stderr, "bad band: %s\n", argv[i]); return 2; }
            bands.push_back(b);
        }
        const int total_pairs = (int)bands.size() * SkipGeom::V3_ROWS, n_pass = (total_pairs + SkipGeom::RPP - 1) / SkipGeom::RPP;
        for (int p = 0; p < n_pass; ++p)
            std::putchar(skip_pass_needed(p, total_pairs, [&](const int crop) { return bands.at((size_t)crop); }) ? '1' : '0');
        std::putchar('\n');
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, (int)std::atoll(argv[2]), std::atoi(argv[3]), 256);
        std::printf("chain=%d skip=%d\n", (int)p.chain, (int)p.skip);
        return 0;
    }
    std::fprintf(stderr, "usage: rows | passes y0:y1 ... | plan geom n\n");
    return 2;
}
