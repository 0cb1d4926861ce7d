// Prints what the rule of the listed fc1 (skip3_fc1_listed, trex_amd/csrc/cnn_skip3.h) says, and the per-plane crop lists a host restatement of
// k_fc1_list's compaction (cnn_skip_kernels.h: 64 crops to a bit-map word, a count per word, an exclusive scan, every set bit written behind the
// set bits in front of it) makes of a batch of bands; tests/test_fc1_list.py holds both to a brute-force propagation of dependence.
//   rule all                     "y0 y1 mask" for no non-zero row (y0 = 80, y1 = -1) and every 0 <= y0 <= y1 < 80; bit q of mask: plane q is listed
//   lists all y0:y1 y0:y1 ...    one crop per argument (80:-1: an empty crop); one line per plane: "q len: crop crop ..."
//   plan geom n                  "fc1_listed=<0|1> fc1=<0 exact, 1 split1, 2 split4> head=<0 small, 1 big> fill=<k_act3_fill's grid>" on 256 CUs
// all: 1 = the empty crop left the fp16 range (the word SK_EMPTY_RANGE is set), 0 = it did not
#include "../../trex_amd/csrc/cnn_plan.h"
#include "../../trex_amd/csrc/cnn_skip_words.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace trexhip;

static_assert(!skip3_fc1_listed(false, SKIP_BAND_NONE, 0) && skip3_fc1_listed(true, SKIP_BAND_NONE, 9), "usable in constant expressions");
static_assert(skip3_fc1_listed(false, {0, 79}, 0) && skip3_fc1_listed(false, {0, 79}, Skip3Geom::PAIRS - 1), "a full crop lists every plane");
static_assert(SK3_FC1_LEN > SK3_EMPTY_CTR && SK3_FC1_LEN > SK3_FC1E_RANGE && SK3_LAST == SK3_FC1_LEN + 9, "the lengths lie behind the other words");

static unsigned mask_of(const bool all, const SkipBand b) {
    unsigned m = 0;
    for (int q = 0; q < Skip3Geom::PAIRS; ++q) m |= (unsigned)skip3_fc1_listed(all, b, q) << q;
    return m;
}

// the compaction, as the kernel does it for one plane
static std::vector<int> plane_list(const bool all, const std::vector<SkipBand>& bands, const int q) {
    const int n = (int)bands.size(), nw = (n + 63) / 64;
    std::vector<uint64_t> mask(nw, 0);
    for (int w = 0; w < nw; ++w)
        for (int lane = 0; lane < 64; ++lane) {
            const int crop = w * 64 + lane;
            if (crop < n && skip3_fc1_listed(all, bands[crop], q)) mask[w] |= 1ull << lane;
        }
    std::vector<uint32_t> off(nw + 1, 0);
    for (int w = 0; w < nw; ++w) off[w + 1] = off[w] + (uint32_t)__builtin_popcountll(mask[w]);
    std::vector<int> list(off[nw], -1);
    for (int w = 0; w < nw; ++w)
        for (int lane = 0; lane < 64; ++lane)
            if ((mask[w] >> lane) & 1ull) list[off[w] + (uint32_t)__builtin_popcountll(mask[w] & ((1ull << lane) - 1ull))] = w * 64 + lane;
    return list;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "rule")) {
        const bool all = std::atoi(argv[2]) != 0;
        std::printf("%d %d %u\n", SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1, mask_of(all, SKIP_BAND_NONE));
        for (int y0 = 0; y0 < SkipGeom::CROP_ROWS; ++y0)
            for (int y1 = y0; y1 < SkipGeom::CROP_ROWS; ++y1) std::printf("%d %d %u\n", y0, y1, mask_of(all, {y0, y1}));
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "lists")) {
        const bool all = std::atoi(argv[2]) != 0;
        std::vector<SkipBand> bands;
        for (int i = 3; i < argc; ++i) {
            int y0, y1;
            if (std::sscanf(argv[i], "%d:%d", &y0, &y1) != 2 || y0 < 0 || y0 > SkipGeom::CROP_ROWS || y1 < -1 || y1 >= SkipGeom::CROP_ROWS) {
                std::fprintf(stderr, "bad band: %s\n", argv[i]);
                return 2;
            }
            bands.push_back({y0, y1});
        }
        for (int q = 0; q < Skip3Geom::PAIRS; ++q) {
            const std::vector<int> list = plane_list(all, bands, q);
            std::printf("%d %zu:", q, list.size());
            for (const int c : list) std::printf(" %d", c);
            std::printf("\n");
        }
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, (int)std::atoll(argv[2]), std::atoi(argv[3]), 256);
        std::printf("fc1_listed=%d fc1=%d head=%d fill=%d\n", (int)p.fc1_listed, (int)p.fc1, (int)p.head, p.act3_fill.grid);
        return 0;
    }
    std::fprintf(stderr, "usage: rule all | lists all y0:y1 ... | plan geom n\n");
    return 2;
}
