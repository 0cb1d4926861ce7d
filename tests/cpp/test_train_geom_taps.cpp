// Prints what the tap count changes in the geometry of the any-size training chain (trex_amd/csrc/train_geom.h), one line per argument:
//   W,H,CH,n,taps   ->   name=value pairs; taps = 0 calls train_any_geom(W, H, CH) without the argument (the default)
// tests/test_train_geom_taps.py holds the lines to numbers derived by hand.
#include "../../trex_amd/csrc/train_geom.h"
#include <cstdio>

using namespace trexhip;

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        int W, H, CH, n, taps;
        if (std::sscanf(argv[i], "%d,%d,%d,%d,%d", &W, &H, &CH, &n, &taps) != 5) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const TrainAnyGeom g = taps ? train_any_geom(W, H, CH, taps) : train_any_geom(W, H, CH);
        std::printf("taps=%d z3=%dx%d P=%d conv2=%d,%d,%d conv3=%d,%d,%d wgrad1=%d,%d wgrad2=%d,%d,%d wgrad3=%d,%d,%d part=%zu part1=%zu z=%zu a=%zu f1w=%zu\n", g.taps,
                    g.L[2].w, g.L[2].h, g.P, g.L[1].tiles.TX, g.L[1].tiles.tx_n, g.L[1].tiles.tiles, g.L[2].tiles.TX, g.L[2].tiles.tx_n, g.L[2].tiles.tiles,
                    g.wg1_tx, g.wg1_tiles, g.L[1].wg_types, g.wg_per(1, n), g.wg_shares(1, n), g.L[2].wg_types, g.wg_per(2, n), g.wg_shares(2, n),
                    4 * g.part_floats(), 4 * g.part1_floats(n), 4 * g.z_floats(2, n), 4 * g.a_floats(2, n), 4 * g.fc1_weight_floats());
    }
    return 0;
}
