// cnn_net.h -- the identity network's host state and how its kernels are launched, shared by cnn.hip and cnn_any.hip (not part of the ABI)
#pragma once
#include "internal.h"
#include "cnn_plan.h"
#include "cnn_skip.h"
#include "cnn_skip_words.h"
#include "cnn_skipx.h"
#include <tuple>

namespace trexhip {

struct ArchNet;      // cnn_arch.h

struct Net {
    int classes = 0, W = 0, H = 0, CH = 0, max_crops = 0;
    ArchNet* arch = nullptr;                   // v100 / v110 / v119 / v200: the network's own state (cnn_arch.hip); of the fields below it uses the guard
                                               // words, the per-crop flags, crops / probs / logits / h_probs and the two owners.  Null: V118_3
    uint4 *w2s = nullptr, *w3s = nullptr;      // bf16-split conv weights
    uint4 *w2h = nullptr, *w3h = nullptr;      // fp16-split conv weights (scaled by a power of two)
    float inv2h = 1.f, inv3h = 1.f;
    uint4 *w2w = nullptr, *w3w = nullptr;      // Winograd F(4,5)-domain conv weights, fp16 pieces (k_conv5_wino)
    float inv2w = 1.f, inv3w = 1.f;
    uint4* wf1h = nullptr;                     // fc1 weights, fp16 pieces in MFMA B layout [K/8][2][128] x 8 halves
    float invf1h = 1.f;
    uint4* w1h = nullptr;                      // conv1 B fragments (16 fragments x 64 lanes), fp16 pieces of the folded weights
    float inv1h = 1.f;
    uint32_t* d_ovf = nullptr;                 // the guard words, OVF_WORDS of them (cnn_geom.h: OVF_RANGE, OVF_PASS3, OVF_PASS2, OVF_PLAN)
    uint8_t* d_ovfc = nullptr;                 // per-crop range flags [max_crops]
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;      // folded fp32: conv1 [CH][25][16], conv2 / conv3 chunked
    float *wf1 = nullptr, *bf1 = nullptr, *lng = nullptr, *lnb = nullptr, *wf2t = nullptr, *bf2 = nullptr;
    float *act1 = nullptr, *act2 = nullptr, *act3 = nullptr, *fc1 = nullptr, *probs = nullptr, *logits = nullptr;   // act: [n][H/2][W/2][16], [n][H/4][W/4][64], [n][H/8][W/8][128]
    uint8_t *v2 = nullptr, *v3 = nullptr;      // Winograd-domain operand images of conv2 / conv3 (fp16 pieces), written by the producing layer (cnn_wpre.h)
                                               // (v3: a copy of v3e lies in front of it and behind its max_crops * 20 rows, where v3e exists)
    uint8_t* crops = nullptr;
    // skipping the passes of k_conv12_rs whose crop rows are all background (cnn_skip.h, cnn_skip_kernels.h; the words of d_skip: cnn_skip_words.h)
    uint8_t* v3e = nullptr;                    // the V3 image of an all-zero crop [20][V3_ROWB], made when the weights are loaded (1 channel, 80 x 80)
    uint32_t* d_skip = nullptr;                // SK_WORDS words: the empty crop's range flag, the last call's list length and counters
    int2* skip_bands = nullptr;                // [max_crops] first / last non-zero row
    uint32_t* skip_counts = nullptr;           // per SKIP_LB passes / crops: full-width passes, aligned needed passes, windowed passes, windowed crops
    int* skip_list = nullptr;                  // the full-width passes to compute, in order, + the SKIP_PAD entry behind them
    // the windowed conv1+conv2 (cnn_skipx.h)
    float* act2e = nullptr;                    // the pooled conv2 activations of an all-zero crop [20][20][64], made by the run that makes v3e
    int2* skipx_cols = nullptr;                // [max_crops] first / last non-zero column
    int* skipx_list = nullptr;                 // the windowed passes (skipx_pack), in order, + the SKIP_PAD entry behind them
    uint4* bgtab = nullptr;                    // the background row of the windowed instance as its first tile t0 = 0, 1, 2 sees it: the LDS slot's bytes (cnn_fused12rs.h)
    int* skipx_rows = nullptr;                 // beside every entry of skipx_list: the V2 rows of its crop that are made (skipx_v2_pack)
    // computing only the row pairs of conv3 whose V3 rows hold more than background (cnn_skip3.h, cnn_skip_kernels.h)
    float* act3e = nullptr;                    // the act3 of an all-zero crop [10][10][128], made when the weights are loaded, behind v3e
    uint4* skip3_counts = nullptr;             // per workgroup of k_pair_count: full-width listed passes, pairs, windowed passes, windowed crops
    uint32_t* skip3_tcounts = nullptr;         // full-width and windowed listed passes per block of Skip3Geom::BLOCK crops
    int* skip3_desc = nullptr;                 // Skip3Geom::DESC words per listed pass
    uint32_t* skip3_rows = nullptr;            // Skip3Reach::WORDS words per listed pass: where the rows it stages come from
    int* skip3x_desc = nullptr;                // Skip3XGeom::DESC words per windowed listed pass (skip3_window)
    uint32_t* skip3x_rows = nullptr;           // Skip3Reach::WORDS words per windowed listed pass
    // fc1 computing only the listed (crop, plane) rows (skip3_fc1_listed, cnn_skip3.h)
    float* fc1e = nullptr;                     // the fc1 planes of an all-zero crop [FC1_KSPLIT][128] (plane 0 with the bias), made behind act3e
    int* fc1_list = nullptr;                   // [Skip3Geom::PAIRS][max_crops]: per plane the crops it computes, in order (lengths: d_skip + SK3_FC1_LEN)
    int last_fc1_n = 0;                        // crops of the last forward pass if its fc1 was the listed form, else 0 (trexhip_identify_fc1_stats)
    float* h_probs = nullptr;                  // pinned
    Mem weights, batch;                        // every allocation behind the pointers above: made at load / sized by max_crops (ensure_act)
    // small batches are launch-bound (one frame's 100 crops: 60 us of convolutions in a 160 us chain of ~12 launches): the chain of one
    // identify call is captured into a hipGraph per (buffers, n, precision) and replayed
    // A chain is only captured once the same (buffers, n, precision) key has come THREE times: in tracking the blob count changes from
    // batch to batch, and capture + instantiate costs far more than the ~100 us of launch overhead a replay saves.
    using GraphKey = std::tuple<const uint8_t* /*crops*/, int /*n*/, float* /*probs*/, float* /*logits*/, int /*mode*/, int /*geom*/, hipStream_t>;
    struct GraphEntry { GraphKey key; hipGraphExec_t exec; uint64_t used; hipEvent_t last; int seen; };      // exec == nullptr: a candidate key that is still being counted
    std::vector<GraphEntry> graphs;
    bool graphs_ok = true;
    uint64_t tick = 0;
    bool ovf_clean = true;                     // the words in front of OVF_PLAN are zero, or will be when the queued work has run (see net_forward)
    int last_mode = -1;                        // precision mode of the last forward pass (trexhip_identify_guard_stats reads the plan only behind an fp16x3 pass)
    uint32_t* ovf(const int word) const { return d_ovf + word; }
};

// A kernel instance, stated once with its workgroup size and its dynamic LDS bytes.  An instance that needs the dynamic-LDS attribute lists itself
// when it is constructed (they are file-scope constants); the attribute pass (net_forward_launch) walks that list, and the launch uses the same entry.
struct LdsAttr { const void* fn; int bytes; };
std::vector<LdsAttr>& lds_attrs();
template <class... A>
struct Kern {
    void (*fn)(A...);
    int threads, lds;
    Kern(void (*f)(A...), const int threads_, const int lds_ = 0, const bool attr = true) : fn(f), threads(threads_), lds(lds_) {
        if (lds && attr) lds_attrs().push_back({reinterpret_cast<const void*>(f), lds});
    }
    template <class... B>
    void operator()(hipStream_t s, const dim3 grid, B... args) const { hipLaunchKernelGGL(fn, grid, dim3(threads), lds, s, static_cast<A>(args)...); }
};
// the instances for 1 and for 3 input channels share a signature
template <class K> struct ByChannels {
    K one, three;
    const K& operator[](const int CH) const { return CH == 1 ? one : three; }
};
template <class K> ByChannels(K, K) -> ByChannels<K>;

// the any-size chain's convolutions (cnn_any.hip): conv1 in exact fp32, conv2 (layer 2) / conv3 (layer 3) in the precision mode; with a guard
// (the re-run plan) on the plan's small grid
void any_conv1(hipStream_t s, const Net& net, const CnnPlan& p, const uint8_t* d_crops);
void any_conv(hipStream_t s, const Net& net, const CnnPlan& p, int layer, int mode, const uint32_t* guard);

}  // namespace trexhip
