// Prints where the listed conv3 takes the rows of its passes from (skip3_row_sources / skip3_row_words, trex_amd/csrc/cnn_skip3.h);
// tests/test_cnn_skip3_rows.py holds every line to a brute-force propagation of dependence.
//   scan first total y0:y1 ...   for every band A (none, then every 0 <= y0 <= y1 < 80) two crop sequences, [A, B...] and [B..., A], B... the bands
//                                given; the first crop of a sequence is crop `first` of a batch of `total` crops.  One line per listed pass:
//                                "<crop a> <y0 y1 of a> <crop b> <y0 y1 of b> | <DESC words> | <NR sources> | <WORDS words>"
//                                (crop b = crop a where the pass has one run)
//   fits rows                    "1" when a batch of that many V3 rows lets every pass reach an image, else "0"
//   plan geom n                  "skip3=<0|1> direct=<0|1>" on 256 CUs
#include "../../trex_amd/csrc/cnn_plan.h"
#include "../../trex_amd/csrc/cnn_skip3.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace trexhip;

static constexpr bool sources_by_hand() {
    // crop 1's pairs 3 .. 6 alone in a pass: rows 4 .. 15; own rows 6 .. 11 -> two image rows, six of V3, four image rows, none behind
    Skip3Pass p{};
    p.n = 4; p.runs = 1; p.gp0[0] = 13; p.len[0] = 4;
    int src[Skip3Geom::NR] = {};
    skip3_row_sources(p, SkipRows{6, 11}, SkipRows{1, 0}, src);
    bool ok = src[0] == (S3_SRC_IMAGE | 4) && src[1] == (S3_SRC_IMAGE | 5) && src[2] == 26 && src[7] == 31 && src[8] == (S3_SRC_IMAGE | 12);
    return ok && src[11] == (S3_SRC_IMAGE | 15) && src[12] == S3_SRC_NONE && src[Skip3Geom::NR - 1] == S3_SRC_NONE;
}
static_assert(sources_by_hand(), "usable in constant expressions");
static_assert(skip3_direct_fits(25600ll * 20) && !skip3_direct_fits(40000ll * 20), "the benchmark's batch fits, 8 GB of V3 does not");

int main(int argc, char** argv) {
    using G = Skip3Geom;
    using R = Skip3Reach;
    if (argc >= 4 && !std::strcmp(argv[1], "scan")) {
        const int first = std::atoi(argv[2]);
        const long long total = std::atoll(argv[3]) * SkipGeom::V3_ROWS;
        std::vector<SkipBand> others;
        for (int i = 4; i < argc; ++i) {
            SkipBand b{};
            if (std::sscanf(argv[i], "%d:%d", &b.y0, &b.y1) != 2) { std::fprintf(stderr, "bad band: %s\n", argv[i]); return 2; }
            others.push_back(b);
        }
        std::vector<SkipBand> seq;
        auto emit = [&](const int, const Skip3Pass& p) {
            const int ca = p.gp0[0] / G::PAIRS, cb = p.runs > 1 ? p.gp0[1] / G::PAIRS : ca;
            const SkipBand ba = seq[ca - first], bb = seq[cb - first];
            int d[G::DESC], src[G::NR];
            unsigned w[R::WORDS];
            skip3_describe(p, d);
            skip3_row_sources(p, skip_rows(ba), skip_rows(bb), src);
            skip3_row_words(p, skip_rows(ba), skip_rows(bb), total, w);
            std::printf("%d %d %d %d %d %d |", ca, ba.y0, ba.y1, cb, bb.y0, bb.y1);
            for (int i = 0; i < G::DESC; ++i) std::printf(" %d", d[i]);
            std::printf(" |");
            for (int i = 0; i < G::NR; ++i) std::printf(" %d", src[i]);
            std::printf(" |");
            for (int i = 0; i < R::WORDS; ++i) std::printf(" %u", w[i]);
            std::printf("\n");
        };
        auto walk = [&]() {
            Skip3Pass p{};
            int passes = 0;
            for (size_t c = 0; c < seq.size(); ++c) {
                const SkipPairs r = skip3_pairs(seq[c]);
                if (r.lo <= r.hi) skip3_add_run(p, passes, (first + (int)c) * G::PAIRS + r.lo, r.hi - r.lo + 1, emit);
            }
            skip3_flush(p, passes, emit);
        };
        for (int y0 = -1; y0 < SkipGeom::CROP_ROWS; ++y0)
            for (int y1 = y0 < 0 ? -1 : y0; y1 < (y0 < 0 ? 0 : SkipGeom::CROP_ROWS); ++y1) {
                const SkipBand a = y0 < 0 ? SKIP_BAND_NONE : SkipBand{y0, y1};
                seq.assign(1, a);
                seq.insert(seq.end(), others.begin(), others.end());
                walk();
                seq = others;
                seq.push_back(a);
                walk();
            }
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "fits")) {
        std::printf("%d\n", (int)skip3_direct_fits(std::atoll(argv[2])));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, (int)std::atoll(argv[2]), std::atoi(argv[3]), 256);
        std::printf("skip3=%d direct=%d\n", (int)p.skip3, (int)p.v3_direct);
        return 0;
    }
    std::fprintf(stderr, "usage: scan first total y0:y1 ... | fits rows | plan geom n\n");
    return 2;
}
