// cnn_plan.h -- which kernels one forward pass of the identity network launches, and on which grids: decided once per call by a pure function,
// launched in order by net_forward_launch (cnn.hip).  No device code and no HIP: tests/cpp/test_cnn_plan.cpp holds it to hand-derived numbers.
#pragma once
#include <algorithm>
#include "../../include/trexhip.h"
#include "cnn_geom.h"
#include "cnn_skip_words.h"
#include "cnn_skipx.h"

namespace trexhip {

// the bits of TREXHIP_CONV_GEOM (a test hook; include/trexhip.h documents the values)
enum : int {
    GEOM_FP32_ACT = 0xfff,            // bits 0-11, any of them: the fp32-activation chain
    GEOM_PAIR_SLOTS = 1 << 20,        // the listed conv3 walks passes of pair slots (6 or 10 whole pairs), not of tile slots
    GEOM_NO_SKIP3X = 1 << 21,         // no crop gets a window of conv3 tiles
    GEOM_NO_BGROWS = 1 << 22,         // the windowed conv1+conv2 makes every V2 row, background rows too
    GEOM_NO_SKIPX = 1 << 23,          // no crop gets a window
    GEOM_DENSE_FC1 = 1 << 24,         // the dense fc1
    GEOM_V3_COPY = 1 << 25,           // the listed conv3 reads every row from V3
    GEOM_DENSE_CONV3 = 1 << 26,       // the dense conv3 alone
    GEOM_NO_SKIP = 1 << 27,           // conv1+conv2 computes every pass
    GEOM_TWO_KERNEL = 1 << 28,        // conv1 and conv2 as two kernels
    GEOM_ROLE_SPLIT = 1 << 29,        // the role-split conv1+conv2 at any batch size
    GEOM_FUSED_2WG = 1 << 30,         // the two-workgroup conv1+conv2 at any batch size
    GEOM_MASK = GEOM_FP32_ACT | GEOM_PAIR_SLOTS | GEOM_NO_SKIP3X | GEOM_NO_BGROWS | GEOM_NO_SKIPX | GEOM_DENSE_FC1 | GEOM_V3_COPY | GEOM_DENSE_CONV3 | GEOM_NO_SKIP | GEOM_TWO_KERNEL | GEOM_ROLE_SPLIT | GEOM_FUSED_2WG
};

// 80 x 80, TREXHIP_CNN_FP16X3 (the operand images V2 / V3 are written by the producing layer, cnn_wpre.h):
//   ROLE_SPLIT  k_conv12_rs (conv1 inside conv2, one workgroup per CU)   -> k_conv5_wpair       1 channel, aligned crops, >= 3200 crops
//               In front of it, the preparation that lets the chain skip background (launch_skip_prep, cnn_skip_kernels.h), every part with its
//               switch in TREXHIP_CONV_GEOM:
//                 skip        k_crop_bands, k_pass_count, k_pass_list, k_v3_fill: conv1+conv2 walks a list of the passes that hold a blob's rows, the
//                             V3 rows of the others are the empty crop's.  Off (GEOM_NO_SKIP, bit 27): none of this chain's preparation runs
//                 skipx       k_crop_bands writes the column bands as well and k_pass_list makes TWO lists -- the windowed passes (8 tiles x up to 4
//                             row pairs of one crop) of the crops whose blob fits 8 tiles, the aligned full-width passes the other crops need;
//                             k_conv12_rs<W12XGeom> runs on the first in front of k_conv12_rs<W12RGeom> on the second.  Off (GEOM_NO_SKIPX, bit
//                             23): no crop gets a window -- the same three kernels, one list, the full-width instance alone
//                 bgrows      k_pass_list writes, beside every windowed pass, the V2 rows of its crop that have a non-zero crop row under them
//                             (skipx_v2_rows): the windowed instance's producers make only those, its consumers read the others from a
//                             background slot, filled from a table that instance wrote when the weights were loaded.  Off (GEOM_NO_BGROWS,
//                             bit 22): the word says every row, the producers make every new row
//                 skip3       k_pair_count and k_pair_list in front of k_v3_fill; k_act3_fill and BOTH forms of k_conv5_wpair, the dense one and
//                             the one that walks the listed row pairs, behind conv2 -- the word k_pair_list writes names the one that runs, the
//                             other returns at once.  Off (GEOM_DENSE_CONV3, bit 26): the dense conv3 alone
//                 v3_direct   the listed conv3 reads the background rows from the empty crop's image itself and k_v3_fill returns at once where
//                             that form runs.  Off (GEOM_V3_COPY, bit 25): the fill always copies, the listed form reads every row from V3
//                 skip3x      where v3_direct is on: k_pair_count / k_pair_list read the column bands too and make TWO lists of conv3 passes -- windowed
//                             passes (10 row pairs x 3 tiles, skip3_window) of the crops whose blob reaches at most 3 of conv3's 5 tiles, full-width
//                             passes (6 row pairs) of the others; k_act3_fill describes both and copies the pooled columns outside the windows;
//                             k_conv5_wpair<true, Skip3XGeom> runs on the first list in front of the full-width listed instance on the second.  Off
//                             (GEOM_NO_SKIP3X, bit 21): no crop gets a window -- the same kernels, one list, the full-width listed instance alone
//                 skip3t      a listed pass of either list is up to 64 CONSECUTIVE TILES of the list's pair sequence (cnn_skip3.h: Skip3TGeom,
//                             Skip3TXGeom), begun and ended at any even tile of a pair: k_pair_count<true> / k_pair_list<true> / k_act3_fill<true>
//                             make those lists (and still count the passes of pair slots, which the counters and the choice of the form keep
//                             to), the instances k_conv5_wpair<true, Skip3TGeom> and <true, Skip3TXGeom> walk them.  Off (GEOM_PAIR_SLOTS, bit 20):
//                             passes of 6 (10) whole pairs, 60 of the kernel's 64 tiles
//                 fc1_listed  above 1024 crops: k_fc1_list beside k_pair_list, fc1 computes only the (crop, split-K plane) rows whose row pair is
//                             listed -- the listed k_fc1_split<4>; k_head takes the other planes from the empty crop's, k_act3_fill copies no
//                             pair.  Off (GEOM_DENSE_FC1, bit 24): the dense fc1, and the fill copies
//   FUSED_2WG   k_conv12_wpre (the same, two workgroups per CU)          -> k_conv5_wpair       1 channel, aligned crops, fewer
//   TWO_KERNEL  k_conv1_wpre -> k_conv2_wpre2                            -> k_conv5_wpair       3 channels, or TREXHIP_CONV_GEOM bit 28
//   FP32_ACT    conv1 -> act1 -> k_conv5_stream -> act2 -> k_conv5_wino                         unaligned crops, or any of bits 0-11
// 80 x 80, the other modes:  EXACT  conv1 -> k_conv5 (FP32) / k_conv5_split (BF16X6, BF16X3) for conv2 and conv3
// every other size:          ANY_SIZE  k_any_conv1 -> k_any_conv<mode> x 2 (cnn_any.hip)
enum class Chain { ROLE_SPLIT, FUSED_2WG, TWO_KERNEL, FP32_ACT, EXACT, ANY_SIZE };
enum class Conv1 { FUSED /* none of its own */, WPRE, MFMA, VALU, ANY };
enum class Fc1 { EXACT /* k_fc1 */, SPLIT1 /* k_fc1_split<1> */, SPLIT4 /* k_fc1_split<4> */ };
enum class Head { SMALL /* k_head_small */, BIG /* k_head */ };

// items: what the kernel walks (workgroups' worth of work, or the passes of a persistent kernel); grid: the workgroups that go out
struct Launch { int grid, items; };

struct CnnPlan {
    Chain chain;
    Conv1 conv1;
    int conv1_grid;
    Launch conv2, conv3;            // of the kernels the chain names
    int pk2;                        // consecutive passes per ticket of the fused conv1+conv2 kernel, either form
    int n_big3;                     // k_conv5_wpair: tickets of 4 passes in front of the single ones
    Fc1 fc1;
    int fc1_grid, planes, K;        // grid (fc1_grid, planes): split-K planes, summed in the head
    Head head;
    int head_grid;
    // FP16X3 only: the guarded re-run.  Every workgroup of it returns at once unless an activation left the fp16 range; the plan lists the flagged
    // crops (or orders the whole batch when the flag came from a kernel that does not know the crop) and the re-run follows it
    bool rerun;
    bool head_plans;                // k_head_small's first workgroup writes the plan; otherwise k_guard_plan is launched
    bool rerun_conv1;               // the chain left no fp32 activations behind: the re-run starts at the crops (k_conv1_mfma / k_conv1_mfma3)
    Launch r_conv2, r_conv3;        // bf16x6 on the plan: small grids that stride over its crops
    int r_fc1_grid, r_head_grid;    // k_fc1 (r_fc1_grid, planes) and k_head on the plan
    AnyTiles t2, t3;                // ANY_SIZE: tile shapes of conv2 / conv3
    int tx1, t1;                    //           conv1 tiles per row / per crop
    bool skip;                      // ROLE_SPLIT: the passes whose crop rows are all background are not computed (cnn_skip.h); off: TREXHIP_CONV_GEOM bit 27
    bool skip3;                     // where skip is on: conv3 computes only the row pairs that read a row with a blob in it (cnn_skip3.h); off: bit 26
    int skip3_grid;                 // workgroups of k_pair_count / k_pair_list
    Launch act3_fill;               // k_act3_fill: 16 crops (SKIP3_FC) per workgroup
    bool v3_direct;                 // where skip3 is on: the listed conv3 reads background rows from the empty crop's image, k_v3_fill copies only for the
                                    // dense form; off: bit 25, or a batch whose V3 is longer than both images' reach (skip3_direct_fits)
    bool skip3x;                    // where skip3 and v3_direct are on: the listed pairs of the crops whose blob fits a window of 3 conv3 tiles (skip3_window) go
                                    // into windowed passes -- k_pair_count / k_pair_list make two lists, k_act3_fill describes both and copies the pooled columns
                                    // outside the windows, and k_conv5_wpair<true, Skip3XGeom> runs in front of the full-width listed instance; off: bit 21
    bool skip3t;                    // where skip3 is on: the listed passes are 64 consecutive tiles of the list's pairs, not whole pairs; off: bit 20
    bool fc1_listed;                // where skip3 is on, fc1 is SPLIT4 and the head BIG: k_fc1_list in front of conv1+conv2, the listed k_fc1_split<4>
                                    // computes only the listed (crop, plane) rows, k_head takes the others from Net::fc1e, k_act3_fill copies nothing; off: bit 24
    bool skipx;                     // where skip is on: the crops whose blob fits a window of 8 tiles take the windowed instance of the role-split kernel
                                    // (cnn_skipx.h), the others the full-width one, each on its own list, grid conv2.grid and tickets of pk2 slots; off: bit 23,
                                    // or a batch of SKIPX_MAX_CROPS (2^22) crops or more, whose crop index a windowed list entry does not hold
    bool bgrows;                    // where skipx is on: the windowed instance makes only the V2 rows with a non-zero crop row under them; off: bit 22
};

inline int ceil_div(const int a, const int b) { return (a + b - 1) / b; }
inline Launch whole(const int items) { return {items, items}; }      // one workgroup per item
// a guarded re-run is a handful of crops: it goes out on a small grid that strides over them
inline Launch guarded(const int items, const int n_cus) { return {std::min(items, 4 * n_cus), items}; }

inline CnnPlan cnn_plan(const int W, const int H, const int CH, const int mode, const bool aligned, const int geom, const int n, const int n_cus) {
    using GW = WinoGeom<64, 128, 20, 2>;
    CnnPlan p{};
    const bool h16 = mode == TREXHIP_CNN_FP16X3;
    // fc1 split-K planes: the largest count up to FC1_KSPLIT that divides the (H/8)(W/8) positions, so that every plane is whole positions of 128
    // channels (a multiple of k_fc1's 32-deep chunks); 80 x 80: FC1_KSPLIT, which keeps every CU busy at a few thousand crops
    // (25600 crops: 10 planes 344 + 72 us for fc1 + head, 5 planes 319 + 66, 4: 365, 8: 381, 2: 347)
    // (the number of planes must not depend on n -- 5 planes above 12800 crops gave the same crop bit-different probabilities in batches
    // of 12799 and 12800; 10 always costs 31 us of a 9 ms step)
    const int P = (H / 8) * (W / 8);
    p.planes = FC1_KSPLIT;
    while (P % p.planes) --p.planes;
    p.K = 128 * P;
    p.fc1 = Fc1::EXACT;
    p.fc1_grid = p.r_fc1_grid = ceil_div(n, 32);
    p.head = Head::BIG;
    p.head_grid = p.r_head_grid = ceil_div(n, 4 * HEAD_CPW);
    p.rerun = h16;

    if (W != 80 || H != 80) {
        p.chain = Chain::ANY_SIZE;
        p.conv1 = Conv1::ANY;
        p.tx1 = ceil_div(W / 2, C1T);
        p.t1 = ceil_div(H / 2, C1T) * p.tx1;
        p.conv1_grid = n * p.t1;
        p.t2 = any_tiles(H / 4, W / 4);
        p.t3 = any_tiles(H / 8, W / 8);
        p.conv2 = whole(n * p.t2.tiles);
        p.conv3 = whole(n * p.t3.tiles);
        p.r_conv2 = guarded(p.conv2.items, n_cus);
        p.r_conv3 = guarded(p.conv3.items, n_cus);
        return p;
    }

    // the matrix-core conv1 kernels read the crops with 16-byte loads: unaligned crop buffers take the VALU kernel (and the fp32-activation chain)
    // default chain (cnn_wpre.h): the Winograd-domain fp16 operand images V2 / V3 are written by the producing layer.  Any of bits 0-11 of
    // TREXHIP_CONV_GEOM selects the fp32-activation chain of rounds 1-2 instead.
    const bool pre = h16 && aligned && (geom & GEOM_FP32_ACT) == 0;
    // one input channel: conv1 runs INSIDE conv2 (cnn_fused12.h: the V2 image stays in LDS); TREXHIP_CONV_GEOM bit 28 keeps the two kernels
    const bool fused12 = pre && CH == 1 && !(geom & GEOM_TWO_KERNEL);
    // the role-split form (cnn_fused12rs.h): one workgroup of 8 waves per CU, consumer waves (tap loop, output transform) beside producer waves (V3
    // transform of the previous pass, V2 rows of the next), the first 15 taps' weight fragments resident in LDS.  Bit-identical to the
    // two-workgroups-per-CU kernel and 6 % faster at 25600 crops (3.81 against 4.05 ms on one box); batches that do not give every CU a few
    // passes keep the older kernel (1000 crops: 0.207 against 0.196 ms).  TREXHIP_CONV_GEOM bit 29 forces the role-split kernel, bit 30 the older one
    const bool role_split = fused12 && !(geom & GEOM_FUSED_2WG) && ((geom & GEOM_ROLE_SPLIT) || n >= 3200);
    p.chain = role_split ? Chain::ROLE_SPLIT : fused12 ? Chain::FUSED_2WG : pre ? Chain::TWO_KERNEL : h16 ? Chain::FP32_ACT : Chain::EXACT;
    p.conv1 = fused12 ? Conv1::FUSED : pre ? Conv1::WPRE : aligned ? Conv1::MFMA : Conv1::VALU;
    p.conv1_grid = n;
    p.skip = role_split && !(geom & GEOM_NO_SKIP);
    p.skip3 = p.skip && !(geom & GEOM_DENSE_CONV3);
    p.skipx = p.skip && !(geom & GEOM_NO_SKIPX) && n < SKIPX_MAX_CROPS;
    p.bgrows = p.skipx && !(geom & GEOM_NO_BGROWS);
    if (p.skip3) {
        p.skip3_grid = ceil_div(ceil_div(n, 32 /* Skip3Geom::BLOCK crops per thread */), 256);
        p.act3_fill = {ceil_div(n, 16), n};
        p.v3_direct = !(geom & GEOM_V3_COPY) && skip3_direct_fits((long long)n * SkipGeom::V3_ROWS);
        p.skip3x = p.v3_direct && !(geom & GEOM_NO_SKIP3X) && skip3x_direct_fits((long long)n * SkipGeom::V3_ROWS);
        p.skip3t = !(geom & GEOM_PAIR_SLOTS) && skip3t_direct_fits((long long)n * SkipGeom::V3_ROWS);
    }

    const int n_pass2 = ceil_div(n * 20, W2bGeom::RPP), n_pass3 = ceil_div(n * GW::TPC, GW::MB);
    if (fused12) {
        // passes per ticket: long tickets save the 4 extra rows of a ticket's first pass, short ones keep every workgroup busy when the batch is small
        // (a tail of short tickets was measured and dropped: the dynamic tickets already finish together, and every ticket's first pass produces 10
        // rows instead of 6)
        const int wgs = role_split ? n_cus : 2 * n_cus;
        p.pk2 = std::max(1, std::min(role_split ? 32 : 16, n_pass2 / (wgs * 4)));
        p.conv2 = {std::min(ceil_div(n_pass2, p.pk2), wgs), n_pass2};
    }
    else if (pre) p.conv2 = {std::min(n_pass2, 2 * n_cus), n_pass2};       // two workgroups per CU
    else if (h16) p.conv2 = whole(n * ConvGeomS<16, 64, 40, 8, 4>::BPC);   // 8 output rows per workgroup: 320 pixels = exactly 10 M-tiles, 3 workgroups per CU (1.15 ms; 10 rows: 1.31 ms)
    else if (mode == TREXHIP_CNN_FP32) p.conv2 = whole(n * ConvGeom<16, 64, 40, 20, 16>::BPC);
    else p.conv2 = whole(n * ConvGeomB<16, 64, 40, 10, SPLIT_NP>::BPC);
    if (pre) {
        // tickets of 4 consecutive passes (their halo rows are L2 hits) for the first 7/8 of the passes, single passes behind them; a batch that
        // gives a workgroup fewer than 4 tickets goes out pass by pass altogether (100 crops = 157 passes: 157 workgroups at once instead of 40
        // that walk 4 passes each: 93 -> 35 us)
        p.n_big3 = n_pass3 >= 16 * n_cus ? (int)((long long)n_pass3 * 7 / 8) / 4 : 0;
        p.conv3 = {std::min(p.n_big3 + (n_pass3 - p.n_big3 * 4), n_cus), n_pass3};
    }
    else if (h16) p.conv3 = {std::min(n_pass3, n_cus), n_pass3};           // Winograd F(4,5) along x: 0.4x the matrix work of the direct form
    else if (mode == TREXHIP_CNN_FP32) p.conv3 = whole(n * ConvGeom<64, 128, 20, 20, 32>::BPC);
    else p.conv3 = whole(n * ConvGeomB<64, 128, 20, 20, SPLIT_NP>::BPC);

    // small batches: 32 crops per fc1 workgroup and one crop per wave of the head, nothing but latency to save (same sums in the same order: a
    // crop's row does not depend on the kernels its batch got)
    const bool small = n <= 1024;
    if (h16) {
        p.fc1 = small ? Fc1::SPLIT1 : Fc1::SPLIT4;
        if (!small) p.fc1_grid = ceil_div(n, 128);
    }
    if (small) { p.head = Head::SMALL; p.head_grid = ceil_div(n, 4); }
    p.fc1_listed = p.skip3 && p.fc1 == Fc1::SPLIT4 && p.head == Head::BIG && !(geom & GEOM_DENSE_FC1);
    p.head_plans = h16 && small;
    p.rerun_conv1 = pre;
    p.r_conv2 = guarded(n * ConvGeomB<16, 64, 40, 10, SPLIT_NP>::BPC, n_cus);
    // (conv3 in bands of 4 rows, five workgroups per crop: a re-run is a handful of crops, and one workgroup walking a whole crop's 2 GFLOP
    // alone took 0.4 ms of the 0.5 ms a tripped guard cost)
    p.r_conv3 = guarded(n * ConvGeomB<64, 128, 20, 4, SPLIT_NP>::BPC, n_cus);
    return p;
}

}  // namespace trexhip
