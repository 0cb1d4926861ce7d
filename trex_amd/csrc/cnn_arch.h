// cnn_arch.h -- the identity networks v100, v110, v119 and v200 on the device (cnn_arch.hip): what a loaded one holds, and the three calls
// cnn.hip makes for it.  Not part of the ABI.  The layer table and the plan: cnn_arch_plan.h; the operand images: cnn_weights.h.
// The category network (trex_learn_category.py:18-44) is one more plan of the same chain, held in the context's second slot (ctx->cat) by
// categorize.hip: category_load builds it, arch_ensure_act / arch_forward take the Net they work on.
#pragma once
#include "cnn_net.h"
#include "cnn_arch_plan.h"

namespace trexhip {

// guard words of an architecture net (Net::d_ovf): those of cnn_geom.h, and behind them what the chunks of the last call re-ran together
enum : int { ARCH_STAT_RERUN = OVF_WORDS, ARCH_STAT_WHOLE = OVF_WORDS + 1, ARCH_OVF_WORDS = OVF_WORDS + 2 };

struct ArchLayerDev {
    float* w = nullptr;        // fp32 image (pack_arch_conv / pack_arch_conv1)
    uint4* ws = nullptr;       // bf16 pieces
    uint4* wh = nullptr;       // fp16 pieces of the scaled weights, invh undoes the scale
    float invh = 1.f;
    float *bias = nullptr, *s = nullptr, *t = nullptr;      // the epilogue's per-channel vectors
    float* act = nullptr;      // [chunk][Ho][Wo][CO]
    float* pool = nullptr;     // [chunk][H3][W3][CO] behind k_pool3
};

struct ArchNet {
    ArchPlan plan;
    ArchLayerDev L[5];
    float *wf1 = nullptr, *bf1 = nullptr;      // fc1 [K][NH], bias [NH]
    float *hs = nullptr, *ht = nullptr;        // the head's affine (BatchNorm1d) [NH]
    float *wf2t = nullptr, *bf2 = nullptr;     // fc2 [hidden][classes], bias
    float* gap = nullptr;                      // [chunk][Cf] behind the global average pool
    float* fc1 = nullptr;                      // [chunk][NH]
    int32_t *labels = nullptr, *h_labels = nullptr;      // the category network's host route: [n] on the device, pinned
};

// trexhip_load_weights on a blob whose header names one of the four: parse -> pack -> upload; replaces the context's network
int arch_load(trexhip_ctx* ctx, const void* blob, size_t bytes);
// the buffers of a call of n crops: crops / probabilities by n, activations by min(n, chunk), all from net->batch
int arch_ensure_act(trexhip_ctx* ctx, Net* net, int n, const char* who = "trexhip_identify_device");
// one identify call: the crops in chunks, each chunk the whole chain
int arch_forward(trexhip_ctx* ctx, const Net& net, const uint8_t* d_crops, int n, float* d_probs, float* d_logits, int32_t* d_labels = nullptr);
// trexhip_categorize_load_weights: the category network (trex_learn_category.py:18-44) into ctx->cat; a refused blob leaves the loaded one
int category_load(trexhip_ctx* ctx, const void* blob, size_t bytes);

void free_net(Net* n);      // cnn.hip

}  // namespace trexhip
