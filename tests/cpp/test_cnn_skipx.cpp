// Prints what the column rule, the windows, the packing and the barrier count of the windowed conv1+conv2 (trex_amd/csrc/cnn_skipx.h) say;
// tests/test_cnn_skipx.py holds them to a brute-force propagation and to hand-derived numbers.
//   tiles                        "x0 x1 lo hi" for no non-zero column (x0 = 80, x1 = -1) and for every 0 <= x0 <= x1 < 80
//   window x0 x1 out_of_range    the window's first tile, -1: none
//   windows                      "x0 x1 t0" for every 0 <= x0 <= x1 < 80, the empty crop in range
//   pack crop lo hi t0           the windowed passes of a crop whose needed V3 rows are lo .. hi: "crop r0 rows t0 entry" per pass, unpacked from the entry
//   packs crop t0                "lo hi crop r0 rows t0" per pass, for every run 0 <= lo <= hi < 20
//   full y0:y1:x0:x1 ...         one crop per argument: a line of 0 / 1 per aligned pass of the batch (the full-width list), then the windowed
//                                passes of the batch "crop r0 rows t0", in list order
//   nowin y0:y1 ...              one crop per argument, none of them with a window (win(crop) == -1): two lines of 0 / 1 per aligned pass of the batch,
//                                skip_pass_needed and skipx_full_needed -- the list kernels with no column bands rest on their being equal
//   nowin                        the same for every band (none: 80:-1, and every 0 <= y0 <= y1 < 80) at crops 2, 3 and 4 of a batch of 7 (its rows at
//                                every alignment of a 3-row pass), an empty crop in front of it, a full one behind it: "at y0 y1 bits bits"
//   stages                       "w|f first|next a b new chunks stages": windowed (a = first row r0, b = rows; next: behind a pass of 4 rows of the same
//                                run) and full width (a = pass of a 2-crop batch, b = 0; next: behind pass a - 1)
//   plan geom n                  "chain=<0 for role split> skip=<0|1> skipx=<0|1>" of the 80 x 80 one-channel FP16X3 plan on 256 CUs
#include "../../trex_amd/csrc/cnn_plan.h"
#include "../../trex_amd/csrc/cnn_skipx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace trexhip;

static_assert(skipx_tiles(SKIP_BAND_NONE).lo > skipx_tiles(SKIP_BAND_NONE).hi, "usable in constant expressions");
static_assert(rs_round_stages(0, 8) == 3 && rs_round_stages(8, 8) == 3 && rs_round_stages(9, 8) == 6, "a round has its three stages even with nothing to produce");

// the aligned passes a batch without windows needs, by the row rule alone and by the rule of the two lists
static void nowin_bits(const std::vector<SkipBand>& bands, std::string& rows, std::string& lists) {
    const int total_pairs = (int)bands.size() * SkipGeom::V3_ROWS, n_pass = (total_pairs + SkipGeom::RPP - 1) / SkipGeom::RPP;
    const auto band = [&](const int crop) { return bands.at((size_t)crop); };
    rows.clear();
    lists.clear();
    for (int p = 0; p < n_pass; ++p) {
        rows += skip_pass_needed(p, total_pairs, band) ? '1' : '0';
        lists += skipx_full_needed(p, total_pairs, band, [](int) { return -1; }) ? '1' : '0';
    }
}

static void stage_line(const char* inst, const char* kind, const int a, const int b, const SkipXV2 nw, const int chunk) {
    std::printf("%s %s %d %d %d %d %d\n", inst, kind, a, b, nw.nrows, rs_round_chunks(nw.nrows, chunk), rs_round_stages(nw.nrows, chunk));
}

int main(int argc, char** argv) {
    using X = SkipXGeom;
    if (argc >= 2 && !std::strcmp(argv[1], "tiles")) {
        const SkipTiles none = skipx_tiles(SKIP_BAND_NONE);
        std::printf("%d %d %d %d\n", SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1, none.lo, none.hi);
        for (int x0 = 0; x0 < 80; ++x0)
            for (int x1 = x0; x1 < 80; ++x1) {
                const SkipTiles t = skipx_tiles({x0, x1});
                std::printf("%d %d %d %d\n", x0, x1, t.lo, t.hi);
            }
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "window")) {
        std::printf("%d\n", skipx_window({std::atoi(argv[2]), std::atoi(argv[3])}, std::atoi(argv[4]) != 0));
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "windows")) {
        for (int x0 = 0; x0 < 80; ++x0)
            for (int x1 = x0; x1 < 80; ++x1) std::printf("%d %d %d\n", x0, x1, skipx_window({x0, x1}, false));
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "packs")) {
        for (int lo = 0; lo < SkipGeom::V3_ROWS; ++lo)
            for (int hi = lo; hi < SkipGeom::V3_ROWS; ++hi)
                for (int k = 0; k < skipx_passes({lo, hi}); ++k) {
                    const SkipXPass p = skipx_unpack(skipx_pack(skipx_pass(std::atoi(argv[2]), {lo, hi}, std::atoi(argv[3]), k)));
                    std::printf("%d %d %d %d %d %d\n", lo, hi, p.crop, p.r0, p.rows, p.t0);
                }
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "pack")) {
        const int crop = std::atoi(argv[2]), t0 = std::atoi(argv[5]);
        const SkipRows need{std::atoi(argv[3]), std::atoi(argv[4])};
        for (int k = 0; k < skipx_passes(need); ++k) {
            const int e = skipx_pack(skipx_pass(crop, need, t0, k));
            const SkipXPass p = skipx_unpack(e);
            std::printf("%d %d %d %d %d\n", p.crop, p.r0, p.rows, p.t0, e);
        }
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "full")) {
        std::vector<SkipBand> bands, cols;
        for (int i = 2; i < argc; ++i) {
            SkipBand b, c;
            if (std::sscanf(argv[i], "%d:%d:%d:%d", &b.y0, &b.y1, &c.y0, &c.y1) != 4) { std::fprintf(stderr, "bad crop: %s\n", argv[i]); return 2; }
            bands.push_back(b);
            cols.push_back(c);
        }
        const int n = (int)bands.size(), total_pairs = n * SkipGeom::V3_ROWS, n_pass = (total_pairs + SkipGeom::RPP - 1) / SkipGeom::RPP;
        const auto band = [&](const int crop) { return bands.at((size_t)crop); };
        const auto win = [&](const int crop) { return skipx_window(cols.at((size_t)crop), false); };
        for (int p = 0; p < n_pass; ++p) std::putchar(skipx_full_needed(p, total_pairs, band, win) ? '1' : '0');
        std::putchar('\n');
        for (int c = 0; c < n; ++c) {
            if (win(c) < 0) continue;
            const SkipRows need = skip_rows(band(c));
            for (int k = 0; k < skipx_passes(need); ++k) {
                const SkipXPass p = skipx_unpack(skipx_pack(skipx_pass(c, need, win(c), k)));
                std::printf("%d %d %d %d\n", p.crop, p.r0, p.rows, p.t0);
            }
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "nowin")) {
        std::string rows, lists;
        if (argc > 2) {
            std::vector<SkipBand> bands;
            for (int i = 2; i < argc; ++i) {
                SkipBand b;
                if (std::sscanf(argv[i], "%d:%d", &b.y0, &b.y1) != 2) { std::fprintf(stderr, "bad crop: %s\n", argv[i]); return 2; }
                bands.push_back(b);
            }
            nowin_bits(bands, rows, lists);
            std::printf("%s\n%s\n", rows.c_str(), lists.c_str());
            return 0;
        }
        for (int at = 2; at <= 4; ++at)
            for (int y0 = -1; y0 < 80; ++y0)
                for (int y1 = y0; y1 < (y0 < 0 ? 0 : 80); ++y1) {
                    std::vector<SkipBand> bands(7, SKIP_BAND_NONE);
                    bands[(size_t)at] = y0 < 0 ? SKIP_BAND_NONE : SkipBand{y0, y1};
                    bands[(size_t)at + 1] = {0, SkipGeom::CROP_ROWS - 1};
                    nowin_bits(bands, rows, lists);
                    std::printf("%d %d %d %s %s\n", at, bands[(size_t)at].y0, bands[(size_t)at].y1, rows.c_str(), lists.c_str());
                }
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "stages")) {
        constexpr int V3 = SkipGeom::V3_ROWS;
        // windowed: crop 1 of a batch, so that a mistake in the crop's edges would reach the neighbours' rows
        for (int r0 = 0; r0 < V3; ++r0)
            for (int rows = 1; rows <= X::RPP && r0 + rows <= V3; ++rows) {
                const int gp0 = V3 + r0;
                stage_line("w", "first", r0, rows, rs_new_rows(false, 0, gp0, gp0 + rows - 1), X::CHUNK);
                if (r0 >= X::RPP) {          // behind a pass of RPP rows of the same run
                    const SkipXV2 prev = rs_v2_rows(gp0 - X::RPP, gp0 - 1);
                    stage_line("w", "next", r0, rows, rs_new_rows(true, prev.qmin + prev.nrows, gp0, gp0 + rows - 1), X::CHUNK);
                }
            }
        // full width: every pass of a 2-crop batch (the last one is short), first of a ticket or behind its predecessor
        constexpr int total = 2 * V3, RPP = SkipGeom::RPP, n_pass = (total + RPP - 1) / RPP;
        for (int p = 0; p < n_pass; ++p) {
            const int gp0 = p * RPP, gpl = gp0 + RPP - 1 < total ? gp0 + RPP - 1 : total - 1;
            stage_line("f", "first", p, 0, rs_new_rows(false, 0, gp0, gpl), 6);
            if (p) {
                const SkipXV2 prev = rs_v2_rows(gp0 - RPP, gp0 - 1);
                stage_line("f", "next", p, 0, rs_new_rows(true, prev.qmin + prev.nrows, gp0, gpl), 6);
            }
        }
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "plan")) {
        const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, (int)std::atoll(argv[2]), std::atoi(argv[3]), 256);
        std::printf("chain=%d skip=%d skipx=%d\n", (int)p.chain, (int)p.skip, (int)p.skipx);
        return 0;
    }
    std::fprintf(stderr, "usage: tiles | window x0 x1 range | windows | pack crop lo hi t0 | packs crop t0 | full y0:y1:x0:x1 ... | nowin [y0:y1 ...] | stages | plan geom n\n");
    return 2;
}
