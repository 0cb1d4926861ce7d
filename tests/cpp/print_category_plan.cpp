// print_category_plan.cpp -- prints the launch plan of the category network (category_plan, trex_amd/csrc/cnn_arch_plan.h) for "W,H,CH": per
// layer "L<i>=CI>CO/COBxblocks,t<taps>,p<pool>,HixWi>HoxWo,TX/tx_n/tiles", then fc1 and the chunk.  Host code only.
#include <cstdio>
#include "../../trex_amd/csrc/cnn_arch_plan.h"

int main(int argc, char** argv) {
    int W = 0, H = 0, CH = 0;
    if (argc != 2 || std::sscanf(argv[1], "%d,%d,%d", &W, &H, &CH) != 3) { std::fprintf(stderr, "usage: %s W,H,CH\n", argv[0]); return 2; }
    const trexhip::ArchPlan p = trexhip::category_plan(W, H, CH);
    std::printf("name=%s id=%d n_conv=%d", p.spec->name, p.spec->id, p.n_conv);
    for (int i = 0; i < p.n_conv; ++i) {
        const trexhip::ArchLayerPlan& l = p.L[i];
        std::printf(" L%d=%d>%d/%dx%d,t%d,p%d,%dx%d>%dx%d,%d/%d/%d", i, l.CI, l.CO, l.COB, l.co_blocks, l.taps, l.pool, l.Hi, l.Wi, l.Ho, l.Wo, l.tl.TX, l.tl.tx_n,
                    l.tl.tiles);
    }
    std::printf(" final=%dx%dx%d K=%d NH=%d chunk=%d\n", p.Hf, p.Wf, p.Cf, p.K, p.NH, p.chunk);
    return trexhip::arch_spec(p.spec->id) == nullptr ? 0 : 1;      // the identity table does not know the category network
}
