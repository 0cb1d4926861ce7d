// Prints what trex_amd/csrc/cnn_skipx.h says about the background rows of the windowed conv1+conv2: the V2 rows of a crop that have a non-zero
// crop row under them, and every round of a crop's windowed passes as rs_round gives it to both roles of k_conv12_rs.  tests/test_cnn_bgrows.py
// holds them to a brute-force scan.  Stand-alone, no HIP.
//   v2rows                 for every row band y0 <= y1 < 80: "y0 y1 lo hi" of skipx_v2_rows, and "none lo hi" for a crop without a blob
//   rounds                 for every row band, the windowed passes k of the crop (crop index 3, so that batch rows are not crop rows), each as the
//                          round that makes its rows -- once as it follows its predecessor in the ring ("f"; pass 0 follows nothing), once as a
//                          ticket's first pass ("t"): "y0 y1 k f|t lo hi clo chi chunks stages need_lo"
//                          lo .. chi are V2 rows of the CROP (the crop's first row of the batch subtracted)
//   noclip                 the same rounds with clip = false (the full-width instance, and bit 22 as the device takes it: the range says every
//                          row): "y0 y1 k f|t lo hi clo chi chunks"
//   plan geom n            "skipx=<0|1> bgrows=<0|1>" of the 80 x 80 one-channel FP16X3 plan on 256 CUs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../trex_amd/csrc/cnn_plan.h"

using namespace trexhip;

static_assert(skipx_v2_rows(SKIP_BAND_NONE).lo > skipx_v2_rows(SKIP_BAND_NONE).hi, "usable in constant expressions");
static_assert(skipx_v2_unpack(skipx_v2_pack({7, 39})).lo == 7 && skipx_v2_unpack(skipx_v2_pack({7, 39})).hi == 39, "the word beside a list entry");
static_assert(skipx_v2_unpack(skipx_v2_pack(SKIPX_V2_ALL)).lo == 0 && skipx_v2_unpack(skipx_v2_pack(SKIPX_V2_ALL)).hi == SkipGeom::V2_ROWS - 1, "every row");
// the chunks of a round are a member of the round: a role has no count of rows of its own to call rs_round_chunks with
static_assert(rs_round(false, 0, 60, 63, true, {4, 30}, 8).chunks == rs_round_chunks(rs_round(false, 0, 60, 63, true, {4, 30}, 8).chi - rs_round(false, 0, 60, 63, true, {4, 30}, 8).clo, 8),
              "chunks by the rows made");
static_assert(RS_ROUND_NONE.chunks == rs_round_chunks(0, 8) && RS_ROUND_NONE.lo == RS_ROUND_NONE.hi && RS_ROUND_NONE.clo == RS_ROUND_NONE.chi, "no next pass: one chunk, no rows");

static void rounds(const bool clip) {
    constexpr int CROP = 3, S = SkipGeom::V2_ROWS, CHUNK = SkipXGeom::CHUNK;
    for (int y0 = 0; y0 < 80; ++y0)
        for (int y1 = y0; y1 < 80; ++y1) {
            const SkipRows need = skip_rows({y0, y1});
            const SkipV2 v2 = clip ? skipx_v2_rows({y0, y1}) : SKIPX_V2_ALL;
            int res_hi = 0;
            for (int k = 0; k < skipx_passes(need); ++k) {
                const SkipXPass p = skipx_pass(CROP, need, 0, k);
                const int gp0 = p.crop * SkipGeom::V3_ROWS + p.r0, gpl = gp0 + p.rows - 1;
                for (int f = 1; f >= 0; --f) {
                    const RsRound r = rs_round(f && k > 0, res_hi, gp0, gpl, clip, v2, CHUNK);
                    std::printf("%d %d %d %c %d %d %d %d %d", y0, y1, k, f ? 'f' : 't', r.lo - CROP * S, r.hi - CROP * S, r.clo - CROP * S, r.chi - CROP * S, r.chunks);
                    if (clip) std::printf(" %d %d", rs_round_stages(r.chi - r.clo, CHUNK), need.lo);
                    std::printf("\n");
                    if (!f) res_hi = r.hi;                                   // (the same either way: hi does not depend on `follows`)
                }
            }
        }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "v2rows")) {
        const SkipV2 none = skipx_v2_rows(SKIP_BAND_NONE);
        std::printf("none %d %d\n", none.lo, none.hi);
        for (int y0 = 0; y0 < 80; ++y0)
            for (int y1 = y0; y1 < 80; ++y1) {
                const SkipV2 v = skipx_v2_rows({y0, y1});
                std::printf("%d %d %d %d\n", y0, y1, v.lo, v.hi);
            }
        return 0;
    }
    if (!std::strcmp(argv[1], "plan") && argc == 4) {
        const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, std::atoi(argv[2]) & GEOM_MASK, std::atoi(argv[3]), 256);
        std::printf("skipx=%d bgrows=%d\n", (int)p.skipx, (int)p.bgrows);
        return 0;
    }
    if (!std::strcmp(argv[1], "rounds")) { rounds(true); return 0; }
    if (!std::strcmp(argv[1], "noclip")) { rounds(false); return 0; }
    return 2;
}
