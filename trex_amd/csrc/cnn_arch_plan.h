// cnn_arch_plan.h -- the identity networks v100, v110, v119 and v200 (visual_identification_network_torch.py:30-382) as a layer table, and what one
// identify call on one of them launches: layers, tiles, grids and the chunk its crops are walked in.  Pure host code, no device code and no HIP:
// tests/cpp/test_cnn_arch_plan.cpp holds it to hand-derived numbers.  V118_3 keeps its own plan (cnn_plan.h).
#pragma once
#include <stddef.h>
#include "../../include/trexhip.h"
#include "cnn_geom.h"

namespace trexhip {

// one convolution of a network: 'same', TAPS x TAPS, then (v100, v119, v200) folded BatchNorm + ReLU + pool, or (v110) pool + BatchNorm + ReLU
struct ArchConv {
    int CO;       // output channels of the reference
    int taps;     // 3 or 5
    int pool;     // 0: none; 2: floor 2x2 max-pool inside the convolution's epilogue; 3: floor 3x3 max-pool by k_pool3 behind it
};
struct ArchSpec {
    int id;
    const char* name;
    int min_size;             // smallest W and H: every pool leaves at least one pixel
    int n_conv;
    ArchConv conv[5];
    bool bn2d;                // a BatchNorm2d per convolution ...
    bool bn_behind_pool;      // ... that sits behind the max-pool (v110): its scale may be negative, so it stays a per-channel affine in the epilogue
    bool gap;                 // global average pool in front of fc1 (v200); otherwise the NCHW flatten of the reference
    int hidden;               // fc1 outputs
    bool bn1d;                // BatchNorm1d behind fc1
};

inline const ArchSpec* arch_spec(const int id) {
    static const ArchSpec S[4] = {
        {TREXHIP_NET_V100, "v100", 8, 3, {{16, 5, 2}, {64, 5, 2}, {100, 5, 2}}, false, false, false, 100, false},
        {TREXHIP_NET_V110, "v110", 8, 3, {{16, 5, 2}, {64, 5, 2}, {100, 5, 2}}, true, true, false, 100, true},
        {TREXHIP_NET_V119, "v119", 16, 4, {{256, 5, 2}, {128, 5, 2}, {32, 5, 2}, {128, 5, 2}}, true, false, false, 1024, true},
        {TREXHIP_NET_V200, "v200", 27, 5, {{64, 3, 0}, {128, 3, 3}, {256, 3, 0}, {512, 3, 3}, {512, 3, 3}}, true, false, true, 1024, true},
    };
    return id >= TREXHIP_NET_V100 && id <= TREXHIP_NET_V200 ? &S[id - 1] : nullptr;
}
// The category network (trex_learn_category.py:18-44, PyTorchModel): not an identity network -- it has no TREXHIP_NET_* id, its blob has a magic of
// its own and arch_spec() does not know it.  Three convolutions of 3 taps, each BatchNorm2d -> ReLU -> floor 2x2 max-pool (the BatchNorm in front of
// the pool: folded into weights and bias), the NCHW flatten, fc1 (100) -> ReLU -> fc2; no BatchNorm1d.  Its first layer reads normalised bytes.
static constexpr int ARCH_ID_CATEGORY = -1;
inline const ArchSpec* category_spec() {
    static const ArchSpec S = {ARCH_ID_CATEGORY, "category", 8, 3, {{16, 3, 2}, {64, 3, 2}, {100, 3, 2}}, true, false, false, 100, false};
    return &S;
}
inline const char* arch_name(const int id) { return id == TREXHIP_NET_V118_3 ? "v118_3" : arch_spec(id) ? arch_spec(id)->name : "?"; }

// channels as the kernels see them: 16, or a multiple of 32 (v100 / v110 conv3: 100 -> 128 with zero weights, s = t = 0 behind them)
inline int arch_pad32(const int c) { return c <= 16 ? 16 : (c + 31) / 32 * 32; }
// output channels per workgroup of k_arch_conv: 32 (all 8 waves along M), 64 or 128 (4 waves along N, 2 along M); 256 and 512 channels
// go out as 2 / 4 blocks of 128 on the grid's y
inline int arch_cob(const int CO) { return CO >= 128 ? 128 : CO; }

// the activation budget of one chunk of an identify call, all layers together: a constant, NOT the free memory of the moment, so that the chunk
// -- and with it nothing a crop's row could depend on -- is a pure function of (version, W, H, CH)
static constexpr size_t ARCH_ACT_BUDGET = (size_t)2 << 30;
static constexpr int ARCH_CHUNK_MAX = 1 << 16;     // small crops: bounds the grids (chunk * tiles) far below 2^31

struct ArchLayerPlan {
    int CI, CO;               // padded channels in / out (layer 0: CI = CH)
    int COB, co_blocks;       // output channels per workgroup, blocks on the grid's y
    int taps, pool;
    int Hi, Wi;               // input (= conv output) size
    int Ho, Wo;               // what the convolution kernel writes: Hi/2 x Wi/2 with its fused pool, Hi x Wi without
    AnyTiles tl;              // tile shape in 2x2 windows of conv pixels over ceil(Hi/2) x ceil(Wi/2) (pool 2: over Ho x Wo) and tiles per crop
    int H3, W3;               // pool 3: what k_pool3 writes behind it (otherwise Ho x Wo)
    size_t act_floats;        // per crop: the convolution's output ...
    size_t pool_floats;       // ... and k_pool3's
};

struct ArchPlan {
    const ArchSpec* spec;
    int n_conv;
    ArchLayerPlan L[5];
    int Hf, Wf, Cf;           // what the last layer leaves: Hf x Wf positions of Cf (padded) channels
    int K;                    // fc1's inner size as the kernel walks it: Hf * Wf * Cf in NHWC order, or Cf behind the global average pool
    int NH;                   // fc1 outputs padded to a multiple of 32 (100 -> 128)
    int fc1_planes;           // split-K planes of k_arch_fc1: one -- a function of the layer, never of n (cnn_plan.h on why)
    size_t crop_bytes;        // activation bytes per crop, every buffer of the chain
    int chunk;                // crops per chunk
};

inline int arch_min_size(const int id) { const ArchSpec* s = arch_spec(id); return s ? s->min_size : 8; }

inline ArchPlan arch_plan_of(const ArchSpec* s, const int W, const int H, const int CH) {
    ArchPlan p{};
    p.spec = s;
    p.n_conv = s->n_conv;
    int h = H, w = W, ci = CH;
    size_t floats = 0;
    for (int i = 0; i < s->n_conv; ++i) {
        ArchLayerPlan& l = p.L[i];
        const ArchConv& c = s->conv[i];
        l.CI = ci; l.CO = arch_pad32(c.CO);
        l.COB = i == 0 ? 16 : arch_cob(l.CO);                       // the first layer (k_arch_conv1): 16 channels per workgroup
        l.co_blocks = l.CO / l.COB;
        l.taps = c.taps; l.pool = c.pool;
        l.Hi = h; l.Wi = w;
        const bool p2 = c.pool == 2;
        l.Ho = p2 ? h / 2 : h; l.Wo = p2 ? w / 2 : w;
        const int wy = p2 ? l.Ho : (h + 1) / 2, wx = p2 ? l.Wo : (w + 1) / 2;
        if (i == 0) { const int tx = (wx + C1T - 1) / C1T; l.tl = {C1T, tx, ((wy + C1T - 1) / C1T) * tx}; }
        else l.tl = any_tiles(wy, wx);
        l.H3 = c.pool == 3 ? l.Ho / 3 : l.Ho; l.W3 = c.pool == 3 ? l.Wo / 3 : l.Wo;
        l.act_floats = (size_t)l.Ho * l.Wo * l.CO;
        l.pool_floats = c.pool == 3 ? (size_t)l.H3 * l.W3 * l.CO : 0;
        floats += l.act_floats + l.pool_floats;
        h = l.H3; w = l.W3; ci = l.CO;
    }
    p.Hf = h; p.Wf = w; p.Cf = ci;
    p.K = s->gap ? ci : h * w * ci;
    p.NH = arch_pad32(s->hidden);
    p.fc1_planes = 1;
    floats += (s->gap ? (size_t)ci : 0) + (size_t)p.NH;            // the averaged vector, fc1's output
    p.crop_bytes = floats * 4 + 1;                                   // + the crop's range flag
    const size_t fit = ARCH_ACT_BUDGET / p.crop_bytes;
    p.chunk = fit < 1 ? 1 : fit > (size_t)ARCH_CHUNK_MAX ? ARCH_CHUNK_MAX : (int)fit;
    return p;
}
inline ArchPlan arch_plan(const int id, const int W, const int H, const int CH) { return arch_plan_of(arch_spec(id), W, H, CH); }
inline ArchPlan category_plan(const int W, const int H, const int CH) { return arch_plan_of(category_spec(), W, H, CH); }

}  // namespace trexhip
