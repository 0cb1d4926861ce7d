// Prints the identity network's launch plan (trex_amd/csrc/cnn_plan.h) for the cases on the command line, one per argument:
//   W,H,CH,mode,aligned,geom,n,n_cus   ->   one line of name=value pairs
// tests/test_cnn_plan.py holds the lines to numbers derived by hand.
#include "../../trex_amd/csrc/cnn_plan.h"
#include <cstdio>

using namespace trexhip;

int main(int argc, char** argv) {
    static const char* const chains[] = {"role_split", "fused_2wg", "two_kernel", "fp32_act", "exact", "any_size"};
    static const char* const conv1s[] = {"fused", "wpre", "mfma", "valu", "any"};
    static const char* const fc1s[] = {"k_fc1", "k_fc1_split<1>", "k_fc1_split<4>"};
    static const char* const heads[] = {"k_head_small", "k_head"};
    for (int i = 1; i < argc; ++i) {
        int W, H, CH, mode, aligned, n, n_cus;
        long long geom;
        if (std::sscanf(argv[i], "%d,%d,%d,%d,%d,%lld,%d,%d", &W, &H, &CH, &mode, &aligned, &geom, &n, &n_cus) != 8) {
            std::fprintf(stderr, "bad case: %s\n", argv[i]);
            return 2;
        }
        const CnnPlan p = cnn_plan(W, H, CH, mode, aligned != 0, (int)geom, n, n_cus);
        std::printf("chain=%s conv1=%s conv1_grid=%d conv2=%d/%d pk2=%d conv3=%d/%d n_big3=%d fc1=%s fc1_grid=%d,%d K=%d head=%s head_grid=%d "
                    "rerun=%d head_plans=%d rerun_conv1=%d r_conv2=%d/%d r_conv3=%d/%d r_fc1_grid=%d,%d r_head_grid=%d any=%d,%d,%d,%d,%d\n",
                    chains[(int)p.chain], conv1s[(int)p.conv1], p.conv1_grid, p.conv2.grid, p.conv2.items, p.pk2, p.conv3.grid, p.conv3.items, p.n_big3,
                    fc1s[(int)p.fc1], p.fc1_grid, p.planes, p.K, heads[(int)p.head], p.head_grid, (int)p.rerun, (int)p.head_plans, (int)p.rerun_conv1,
                    p.r_conv2.grid, p.r_conv2.items, p.r_conv3.grid, p.r_conv3.items, p.r_fc1_grid, p.planes, p.r_head_grid, p.t1, p.t2.tiles, p.t2.TX, p.t3.tiles, p.t3.TX);
    }
    return 0;
}
