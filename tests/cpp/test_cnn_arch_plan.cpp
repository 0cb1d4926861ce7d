// The plan of the identity networks v100 / v110 / v119 / v200 (trex_amd/csrc/cnn_arch_plan.h) on the CPU: prints, per argument "id,W,H,CH", the
// layers, tiles, grids' factors and the chunk as key=value pairs (tests/test_cnn_arch_plan.py holds them to hand-derived numbers).  No device call.
#include <cstdio>
#include <cstdlib>
#include "../../trex_amd/csrc/cnn_arch_plan.h"

using namespace trexhip;

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        int id, W, H, CH;
        if (std::sscanf(argv[a], "%d,%d,%d,%d", &id, &W, &H, &CH) != 4 || !arch_spec(id)) { std::fprintf(stderr, "bad case %s\n", argv[a]); return 2; }
        const ArchPlan p = arch_plan(id, W, H, CH);
        std::printf("name=%s min=%d n_conv=%d", p.spec->name, arch_min_size(id), p.n_conv);
        for (int i = 0; i < p.n_conv; ++i) {
            const ArchLayerPlan& l = p.L[i];
            // L<i>=CI>CO/COBxblocks,taps,pool,HixWi>HoxWo>H3xW3,TX/tx_n/tiles
            std::printf(" L%d=%d>%d/%dx%d,t%d,p%d,%dx%d>%dx%d>%dx%d,%d/%d/%d", i, l.CI, l.CO, l.COB, l.co_blocks, l.taps, l.pool, l.Hi, l.Wi, l.Ho, l.Wo, l.H3, l.W3, l.tl.TX,
                        l.tl.tx_n, l.tl.tiles);
        }
        std::printf(" feat=%dx%dx%d K=%d NH=%d planes=%d crop_bytes=%zu chunk=%d\n", p.Hf, p.Wf, p.Cf, p.K, p.NH, p.fc1_planes, p.crop_bytes, p.chunk);
    }
    return 0;
}
