// Prints the geometry of the any-size training chain (trex_amd/csrc/train_geom.h) for the cases on the command line, one per argument:
//   W,H,CH,n   ->   one line of name=value pairs (buffer sizes in bytes at a batch of n)
// and, for the argument "sweep", checks every 8 <= W, H <= 256: tiles, bands and shares cover their planes exactly once, and no count that
// an int holds passes 2^31 at the largest batch.  tests/test_train_geom.py holds the lines to numbers derived by hand.
#include "../../trex_amd/csrc/train_geom.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace trexhip;

// tiles of `size` along one axis, `count` of them: every index of 0..extent-1 in exactly one tile, no tile wholly outside
static bool covers_once(const int extent, const int size, const int count) {
    std::vector<int> hits(extent, 0);
    for (int t = 0; t < count; ++t) {
        if (t * size >= extent) return false;
        for (int k = 0; k < size; ++k)
            if (t * size + k < extent) ++hits[t * size + k];
    }
    for (const int h : hits)
        if (h != 1) return false;
    return true;
}

// `count` contiguous runs of `per` rows: the last one starts inside 0..rows-1 and ends at or past the end
static bool runs_cover(const long long rows, const long long per, const long long count) { return per >= 1 && count * per >= rows && (count - 1) * per < rows; }

static int sweep() {
    const long long LIMIT = 1ll << 31, NMAX = 4096;
    long long checked = 0;
    for (int W = 8; W <= 256; ++W)
        for (int H = 8; H <= 256; ++H) {
            const TrainAnyGeom g = train_any_geom(W, H, 3);
#define FAIL(what) do { std::printf("sweep failed at %dx%d: %s\n", W, H, what); return 1; } while (0)
            if (g.L[0].h != H || g.L[0].w != W || g.L[1].h != H / 2 || g.L[2].w != (W / 2) / 2 || g.h3 != ((H / 2) / 2) / 2 || g.P != g.h3 * g.w3 || g.P < 1 || g.P > 1024)
                FAIL("levels");
            for (int i = 1; i < 3; ++i) {
                const AnyTiles& t = g.L[i].tiles;
                const int hc = (g.L[i].h + 1) / 2, wc = (g.L[i].w + 1) / 2;             // ceil: the odd edge is inside a tile
                if (t.TX != 4 && t.TX != 8 && t.TX != 16) FAIL("tile shape");
                if (t.tiles % t.tx_n || !covers_once(wc, t.TX, t.tx_n) || !covers_once(hc, AW / t.TX, t.tiles / t.tx_n)) FAIL("conv tiles");
                if ((2 * t.TX + 4) * (2 * (AW / t.TX) + 4) > 36 * 12) FAIL("patch");
                for (const long long n : {1ll, 2ll, 7ll, 128ll, NMAX}) {
                    const int per = g.wg_per(i, (int)n), shares = g.wg_shares(i, (int)n);
                    if (shares < 1 || shares > g.L[i].wg_max_shares || !runs_cover(n * g.L[i].h, per, shares)) FAIL("weight-gradient shares");
                }
                if (NMAX * t.tiles >= LIMIT || NMAX * g.L[i].h >= LIMIT) FAIL("grid of a convolution");
            }
            if (g.c1_tiles % g.c1_tx || !covers_once(W, TA_C1T, g.c1_tx) || !covers_once(H, TA_C1T, g.c1_tiles / g.c1_tx)) FAIL("conv1 tiles");
            if (g.wg1_tiles % g.wg1_tx || !covers_once(W, TA_WG1_COLS, g.wg1_tx) || !covers_once(H, TA_WG1_ROWS, g.wg1_tiles / g.wg1_tx)) FAIL("conv1 weight-gradient tiles");
            if (NMAX * g.c1_tiles >= LIMIT || NMAX * g.wg1_tiles >= LIMIT || NMAX * TA_HID >= LIMIT) FAIL("grid");
            // the sizes are size_t: they hold the largest batch, and agree with the products taken in 64 bits
            if (g.z_floats(0, NMAX) != (size_t)(NMAX * H * W * 16) || g.x_floats(NMAX) != (size_t)(NMAX * H * W * 3) ||
                g.a_floats(2, NMAX) != (size_t)(NMAX * g.P * 128) || g.hpart_floats(NMAX) != (size_t)(NMAX * g.P * 100) ||
                g.part1_floats(NMAX) != (size_t)(NMAX * g.wg1_tiles * 1200))
                FAIL("buffer sizes");
#undef FAIL
            ++checked;
        }
    std::printf("sweep ok %lld\n", checked);
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "sweep")) {
            if (const int rc = sweep()) return rc;
            continue;
        }
        int W, H, CH, n;
        if (std::sscanf(argv[i], "%d,%d,%d,%d", &W, &H, &CH, &n) != 4) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const TrainAnyGeom g = train_any_geom(W, H, CH);
        std::printf("z1=%dx%d z2=%dx%d z3=%dx%d a3=%dx%d P=%d conv1=%d,%d conv2=%d,%d,%d conv3=%d,%d,%d wgrad1=%d,%d wgrad2=%d,%d,%d wgrad3=%d,%d,%d "
                    "x=%zu z=%zu,%zu,%zu a=%zu,%zu,%zu hpart=%zu part=%zu part1=%zu f1w=%zu\n",
                    g.L[0].w, g.L[0].h, g.L[1].w, g.L[1].h, g.L[2].w, g.L[2].h, g.w3, g.h3, g.P, g.c1_tx, g.c1_tiles, g.L[1].tiles.TX, g.L[1].tiles.tx_n,
                    g.L[1].tiles.tiles, g.L[2].tiles.TX, g.L[2].tiles.tx_n, g.L[2].tiles.tiles, g.wg1_tx, g.wg1_tiles, g.L[1].wg_types, g.wg_per(1, n),
                    g.wg_shares(1, n), g.L[2].wg_types, g.wg_per(2, n), g.wg_shares(2, n), 4 * g.x_floats(n), 4 * g.z_floats(0, n), 4 * g.z_floats(1, n),
                    4 * g.z_floats(2, n), 4 * g.a_floats(0, n), 4 * g.a_floats(1, n), 4 * g.a_floats(2, n), 4 * g.hpart_floats(n), 4 * g.part_floats(),
                    4 * g.part1_floats(n), 4 * g.fc1_weight_floats());
    }
    return 0;
}
