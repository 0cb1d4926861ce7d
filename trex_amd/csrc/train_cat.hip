// train_cat.hip -- the training step of the category network (trex_learn_category.py:18-44, PyTorchModel, in train mode; the loop body :314-332 on a
// non-CUDA device: fp32 arithmetic.  On `cuda` the reference adds autocast and a GradScaler; that arithmetic is not restated) at every size its blob
// allows: W, H = 8..256, CH = 1 or 3, 1..1024 categories, NHWC fp32, exact fp32 at both values of trexhip_train_params.precision.
//
//   x = byte / 127.5 - 1, zero padded -> [conv3x3 pad 1 -> BatchNorm2d -> ReLU -> MaxPool2 -> Dropout(0.25)] x3 (16, 64, 100 channels)
//     -> flatten (NCHW) -> fc1 (100) -> ReLU -> Dropout(0.25) -> fc2 (categories) -> mean cross entropy; Adam
//
// This file holds no kernel.  The block order is V118_3's, so the chain is train_any.hip's (tany_*) in its 3-tap mode: the conv1 pair normalises its
// input, and the three block kernels read ELEMENT-wise keep masks (the reference uses nn.Dropout on [n][C][h/2][w/2], "Using Dropout instead of
// Dropout2d").  The head is v100's (tarch_head_plain, tarch_head_grads: train_arch.hip), the reductions, Adam, the masks, the target check and the loss
// sum are train.hip's (train_shared.h).  The 100 channels of block 3 travel padded to 128 as in train_arch.hip: a padded slot holds 0 and stays 0 (its
// weights, bias and scale are 0; the block kernels give a channel >= 100 the activation 0 and the gradient 0 whatever its slots hold; Adam's update of
// (p, g, m, v) = 0 is 0).  BatchNorm's statistics run over all n h w pixels of the convolution's plane, the odd last row and column included; block 3's
// plane has at least 2 x 2 pixels at every legal size, so n = 1 trains.  Every sum has a fixed order that depends on the size and n alone; no
// floating-point atomics; one stream.
#include "internal.h"
#include "cnn_weights.h"
#include "train_any.h"
#include "train_shared.h"
#include "train_arch.h"
#include "train_cat.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace trexhip {
namespace {

constexpr int HID = TA_HID, TAPS = 3, T2 = TAPS * TAPS;
constexpr int CP[3] = {16, 64, 128};                     // channels of a block as the kernels see them
constexpr int CR[3] = {16, 64, 100};                     // ... and as torch does
constexpr float P_DROP = 0.25f;                          // nn.Dropout(0.25), all four (trexhip_train_params.dropout is V118_3's)

// the tensors as the trainer holds them: six slots per block (weight, bias, gamma, beta, running mean, running variance), then the head's
enum { S_F1W = 18, S_F1B, S_F2W, S_F2B, S_COUNT };
enum { K_W, K_B, K_G, K_BE, K_RM, K_RV };
// the module's state_dict order (weights.category_shapes): the convolutions, the BatchNorm2d, fc1, fc2
constexpr int ORDER[S_COUNT] = {0, 1, 6, 7, 12, 13, 2, 3, 4, 5, 8, 9, 10, 11, 14, 15, 16, 17, S_F1W, S_F1B, S_F2W, S_F2B};

struct Block {
    int C, CI, creal, h, w, slot;           // z [n][h][w][C]; a, da [n][h/2][w/2][C]; its first tensor slot
    float *z = nullptr, *a = nullptr, *da = nullptr;
    float* wb = nullptr;                    // flipped + transposed weights of its data gradient (blocks 2, 3)
    int cic = 0, dg_co = 0, dg_cic = 0;     // its weight image: the parameter layout's chunk, the data gradient's tile and chunk
};

}  // namespace

struct CatTrainer {
    trexhip_ctx* ctx = nullptr;
    int classes = 0, CH = 1, max_n = 0, W = 0, H = 0;
    TrainAnyGeom geom{};
    trexhip_train_params p{};
    int64_t step = 0;
    size_t off[S_COUNT + 1] = {}, cnt[S_COUNT] = {}, isz[S_COUNT] = {};      // offset, torch's element count, elements held (padded)
    size_t total = 0;
    size_t keep_off[4] = {}, keep_row = 0;  // bytes per sample of the four mask planes: h1 w1 16, h2 w2 64, h3 w3 100, 100
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;
    Block L[3];
    float *part = nullptr, *part1 = nullptr, *stat = nullptr /*3 x (mean, invstd, sums[2]) x 128*/;
    float *hpart = nullptr, *hsum = nullptr, *hd = nullptr, *dl = nullptr, *dh = nullptr, *loss = nullptr, *out2 = nullptr;
    int32_t *correct = nullptr, *bad_target = nullptr;
    double *red = nullptr, *red_bias = nullptr;
    uint8_t *keep = nullptr, *keep_stage = nullptr;
    float* x_stage = nullptr;
    int32_t* y_stage = nullptr;
    Mem mem;
    float* param(int slot) const { return P + off[slot]; }
    float* grad(int slot) const { return G + off[slot]; }
};

namespace {

// index inside the slot, in the kernels' layout, of element `i` of torch's tensor
size_t to_internal(const int slot, const size_t i, const int CH, const size_t P) {
    switch (slot) {
        case 0: { const size_t tap = i % T2, c = (i / T2) % CH, co = i / (T2 * (size_t)CH); return (c * T2 + tap) * 16 + co; }
        case 6: { const size_t tap = i % T2, ci = (i / T2) % 16, co = i / (T2 * 16); return (tap * 16 + ci) * 64 + co; }
        case 12: { const size_t tap = i % T2, ci = (i / T2) % 64, co = i / (T2 * 64); return (((ci / 32) * T2 + tap) * 32 + ci % 32) * 128 + co; }
        case S_F1W: { const size_t K = 100 * P, k = i % K, o = i / K, c = k / P, hw = k % P; return (hw * 128 + c) * HID + o; }      // NCHW flatten
        default: return i;
    }
}

void trainer_free(CatTrainer* t) {
    if (!t) return;
    t->mem.free_all();
    delete t;
}

// plane i of a batch of n starts at keep + n * keep_off[i]
const uint8_t* plane(const CatTrainer* t, const uint8_t* keep, int n, int i) { return keep + (size_t)n * t->keep_off[i]; }

// z -> a of one block.  train: batch statistics over all n h w pixels + the dropout masks; eval: running statistics, the caller's masks keep everything
void block_forward(CatTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* keep, float scale, bool train) {
    const int i = L.slot / 6;
    float* mean = t->stat + i * 512;
    float* invstd = mean + 128;
    if (train) {
        const size_t rows = (size_t)n * L.h * L.w;
        t_bn_stats(s, L.C, L.z, rows, t->red);
        t_fin_bn_stats(s, t->red, T_RED_BLOCKS, L.C, (double)rows, t->p.bn_momentum, mean, invstd, t->param(L.slot + K_RM), t->param(L.slot + K_RV), t->bad_target);
    } else {
        t_bn_from_running(s, t->param(L.slot + K_RM), t->param(L.slot + K_RV), L.C, mean, invstd);
    }
    tany_bn_pool(s, L.C, L.z, mean, invstd, t->param(L.slot + K_G), t->param(L.slot + K_BE), plane(t, keep, n, i), scale, L.a, n, L.h, L.w, L.creal);
}

// da -> dz written over z, the gradients of gamma, beta and the bias; then the weight gradient and the data gradient of blocks 2 and 3
void block_backward(CatTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* keep, float scale) {
    const int i = L.slot / 6;
    const uint8_t* kp = plane(t, keep, n, i);
    float* mean = t->stat + i * 512;
    float* invstd = mean + 128;
    float* sums = mean + 256;
    const float *g = t->param(L.slot + K_G), *be = t->param(L.slot + K_BE);
    tany_pool_bwd_stats(s, L.C, T_RED_BLOCKS, L.da, L.z, mean, invstd, g, be, kp, scale, n, L.h, L.w, t->red, L.creal);
    t_fin_bn_bwd(s, t->red, T_RED_BLOCKS, L.C, sums, t->grad(L.slot + K_G), t->grad(L.slot + K_BE));
    const float inv_count = (float)(1.0 / ((double)n * L.h * L.w));      // the means run over every pixel of the plane
    const int nb = tany_bn_bwd(s, L.C, T_BWD_BLOCKS, L.da, L.z, mean, invstd, g, be, kp, scale, sums, inv_count, n, L.h, L.w, t->red_bias, L.creal);
    t_fin_bias(s, t->red_bias, nb, L.C, t->grad(L.slot + K_B));
    if (i == 0) return;
    const Block& below = t->L[i - 1];
    tany_wgrad(s, t->geom, i, n, below.a, L.z, t->part);
    t_wgrad_reduce(s, t->part, t->geom.wg_shares(i, n), L.CI, L.C, L.cic, t->grad(L.slot + K_W), TAPS);
    t_repack_bwd(s, t->param(L.slot + K_W), L.CI, L.C, L.cic, L.dg_co, L.dg_cic, L.wb, TAPS);
    tany_conv_dgrad(s, t->geom, i, n, L.z, L.wb, below.da);
}

// forward pass up to the per-sample loss / arg-max and the gradient at fc1's output; probs: a prediction
void trainer_forward(CatTrainer* t, hipStream_t s, const float* x, const int32_t* targets, int n, const uint8_t* keep, float scale, bool train, float* probs = nullptr) {
    Block* L = t->L;
    tany_conv1(s, t->geom, n, x, t->param(K_W), t->param(K_B), L[0].z);
    block_forward(t, s, L[0], n, keep, scale, train);
    for (int i = 1; i < 3; ++i) {
        tany_conv_fwd(s, t->geom, i, n, L[i - 1].a, t->param(L[i].slot + K_W), t->param(L[i].slot + K_B), L[i].z);
        block_forward(t, s, L[i], n, keep, scale, train);
    }
    tany_fc1(s, t->geom, n, L[2].a, t->param(S_F1W), t->hpart, t->hsum);
    tarch_head_plain(s, t->hsum, n, t->param(S_F1B), plane(t, keep, n, 3), scale, t->param(S_F2W), t->param(S_F2B), targets, t->classes, t->hd, t->dl, t->dh, t->loss,
                     t->correct, probs);
}

// steps with a target outside 0..categories-1 were refused on the device (k_t_check_targets): train.hip's rule and texts
int check_targets(CatTrainer* t) {
    int32_t bad[2] = {0, 0};
    TH_CHECK_HIP(hipMemcpy(bad, t->bad_target, 8, hipMemcpyDeviceToHost));
    if (bad[0] || bad[1]) {
        TH_CHECK_HIP(hipMemset(t->bad_target, 0, 8));
        if (bad[0]) t->step -= bad[0];
        set_error(bad[0] ? std::string("training step: a target class index was outside 0..classes-1; that step (and the ") + std::to_string(bad[0] - 1) +
                               " queued behind it) was refused, parameters, moments and running statistics are unchanged"
                         : std::string("evaluation batch: a target class index was outside 0..classes-1"));
        return TREXHIP_E_INVALID;
    }
    return TREXHIP_OK;
}

int fetch_loss(CatTrainer* t, hipStream_t s, float* h_loss, int32_t* h_correct) {
    float two[2];
    TH_CHECK_HIP(hipMemcpyAsync(two, t->out2, sizeof(two), hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    if (h_loss) *h_loss = two[0];
    if (h_correct) *h_correct = (int32_t)two[1];
    return check_targets(t);
}

int stage(CatTrainer* t, const char* who, const float* inputs, const int32_t* targets, int n, const uint8_t* keep_masks) {
    for (int i = 0; i < n; ++i)
        if (targets[i] < 0 || targets[i] >= t->classes) { set_error(std::string(who) + ": target class out of range"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(t->ctx->p.device));
    hipStream_t s = t->ctx->stream;
    TH_CHECK_HIP(hipMemcpyAsync(t->x_stage, inputs, (size_t)n * t->H * t->W * t->CH * sizeof(float), hipMemcpyHostToDevice, s));
    TH_CHECK_HIP(hipMemcpyAsync(t->y_stage, targets, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (keep_masks) TH_CHECK_HIP(hipMemcpyAsync(t->keep_stage, keep_masks, (size_t)n * t->keep_row, hipMemcpyHostToDevice, s));
    return TREXHIP_OK;
}

}  // namespace

int cat_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, CatTrainer** out) {
    const char* who = "trexhip_trainer_create";
    ArchBlob ab;
    if (const int rc = parse_category_blob(blob, bytes, who, &ab)) return rc;      // the parser of trexhip_categorize_load_weights: its codes and field names
    if (hipSetDevice(ctx->p.device) != hipSuccess) { set_error("trexhip_trainer_create: hipSetDevice failed"); return TREXHIP_E_DEVICE; }
    CatTrainer* t = new CatTrainer();
    t->ctx = ctx; t->classes = ab.classes; t->CH = ab.CH; t->max_n = p->max_batch; t->p = *p;
    t->W = ab.W; t->H = ab.H;
    t->geom = train_any_geom(ab.W, ab.H, ab.CH, TAPS);
    const size_t P = t->geom.P;
    // ---- the tensors: torch's count and the count held (block 3 and fc1 padded to 128 channels)
    const float* src[S_COUNT] = {};
    for (int i = 0; i < 3; ++i) {
        const size_t ci_r = i ? CR[i - 1] : ab.CH, ci_p = i ? CP[i - 1] : ab.CH;
        t->cnt[6 * i] = (size_t)CR[i] * ci_r * T2; t->isz[6 * i] = (size_t)CP[i] * ci_p * T2;
        for (int k = 1; k < 6; ++k) { t->cnt[6 * i + k] = CR[i]; t->isz[6 * i + k] = CP[i]; }
        for (int k = 0; k < 6; ++k) src[6 * i + k] = ab.conv[i][k];
    }
    t->cnt[S_F1W] = (size_t)HID * 100 * P; t->isz[S_F1W] = t->geom.fc1_weight_floats();
    t->cnt[S_F1B] = t->isz[S_F1B] = HID;
    t->cnt[S_F2W] = t->isz[S_F2W] = (size_t)ab.classes * HID; t->cnt[S_F2B] = t->isz[S_F2B] = ab.classes;
    src[S_F1W] = ab.fc1w; src[S_F1B] = ab.fc1b; src[S_F2W] = ab.fc2w; src[S_F2B] = ab.fc2b;
    size_t at = 0;
    for (int k = 0; k < S_COUNT; ++k) { t->off[k] = at; at += (t->isz[k] + 63) / 64 * 64; }
    t->off[S_COUNT] = at; t->total = at;
    Block* L = t->L;
    size_t krow = 0;
    for (int i = 0; i < 3; ++i) {
        L[i].C = CP[i]; L[i].CI = i ? CP[i - 1] : ab.CH; L[i].creal = CR[i]; L[i].h = t->geom.L[i].h; L[i].w = t->geom.L[i].w; L[i].slot = 6 * i;
        t->keep_off[i] = krow;
        krow += (size_t)(L[i].h / 2) * (L[i].w / 2) * CR[i];
    }
    t->keep_off[3] = krow; t->keep_row = krow + HID;
    L[1].cic = 16; L[1].dg_cic = 16; L[1].dg_co = 32;            // conv2's data gradient: 16 real channels in a 32-wide tile
    L[2].cic = 32; L[2].dg_cic = 32; L[2].dg_co = 64;
    // ---- memory
    const size_t n = (size_t)t->max_n;
    int rc = TREXHIP_OK;
#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)
    TRY(t->mem.device(&t->P, at, who)); TRY(t->mem.device(&t->G, at, who)); TRY(t->mem.device(&t->M, at, who)); TRY(t->mem.device(&t->V, at, who));
    for (int i = 0; i < 3; ++i) {
        const size_t pooled = t->geom.a_floats(i, n);
        TRY(t->mem.device(&L[i].z, t->geom.z_floats(i, n), who)); TRY(t->mem.device(&L[i].a, pooled, who)); TRY(t->mem.device(&L[i].da, pooled, who));
    }
    TRY(t->mem.device(&L[2].wb, (size_t)4 * T2 * 32 * 64, who)); TRY(t->mem.device(&L[1].wb, (size_t)2 * T2 * 32 * 32, who));
    TRY(t->mem.device(&t->part, t->geom.part_floats(), who)); TRY(t->mem.device(&t->part1, t->geom.part1_floats(n), who));
    TRY(t->mem.device(&t->red_bias, (size_t)T_BWD_BLOCKS * 128, who)); TRY(t->mem.device(&t->red, (size_t)T_BWD_BLOCKS * 2 * 128, who));
    TRY(t->mem.device(&t->stat, (size_t)3 * 512, who));
    TRY(t->mem.device(&t->hpart, t->geom.hpart_floats(n), who)); TRY(t->mem.device(&t->hsum, n * HID, who));
    TRY(t->mem.device(&t->hd, n * HID, who)); TRY(t->mem.device(&t->dl, n * ab.classes, who)); TRY(t->mem.device(&t->dh, n * HID, who));
    TRY(t->mem.device(&t->loss, n, who)); TRY(t->mem.device(&t->correct, n, who)); TRY(t->mem.device(&t->out2, 2, who)); TRY(t->mem.device(&t->bad_target, 2, who));
    TRY(t->mem.device(&t->keep, n * t->keep_row, who)); TRY(t->mem.device(&t->keep_stage, n * t->keep_row, who));
    TRY(t->mem.device(&t->x_stage, t->geom.x_floats(n), who)); TRY(t->mem.device(&t->y_stage, n, who));
    TRY(tany_attrs());
#undef TRY
    if (rc != TREXHIP_OK) { trainer_free(t); return rc; }
    std::vector<float> host(at, 0.f);
    for (int k = 0; k < S_COUNT; ++k)
        for (size_t i = 0; i < t->cnt[k]; ++i) host[t->off[k] + to_internal(k, i, ab.CH, P)] = src[k][i];
    bool ok = hipMemcpy(t->P, host.data(), at * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(t->bad_target, 0, 8) == hipSuccess;
    ok = ok && hipMemset(t->G, 0, at * 4) == hipSuccess && hipMemset(t->M, 0, at * 4) == hipSuccess && hipMemset(t->V, 0, at * 4) == hipSuccess;
    if (!ok) { trainer_free(t); set_error("trexhip_trainer_create: upload failed"); return TREXHIP_E_DEVICE; }
    *out = t;
    return TREXHIP_OK;
}

void cat_trainer_destroy(CatTrainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->p.device);
    (void)hipStreamSynchronize(t->ctx->stream);
    trainer_free(t);
}

void cat_trainer_set_lr(CatTrainer* t, float lr) { t->p.lr = lr; }
int64_t cat_trainer_steps(const CatTrainer* t) { return t->step; }
size_t cat_trainer_keep_mask_bytes(const CatTrainer* t, int n) { return (size_t)n * t->keep_row; }
void cat_trainer_info(const CatTrainer* t, int32_t* width, int32_t* height, int32_t* max_batch) {
    if (width) *width = t->W;
    if (height) *height = t->H;
    if (max_batch) *max_batch = t->max_n;
}

int cat_trainer_step(CatTrainer* t, bool host, const float* x, const int32_t* targets, int n, const uint8_t* d_keep, float* h_loss, int32_t* h_correct) {
    const char* who = host ? "trexhip_train_step" : "trexhip_train_step_device";
    if (host) {
        if (const int rc = stage(t, who, x, targets, n, d_keep)) return rc;
        x = t->x_stage; targets = t->y_stage;
        if (d_keep) d_keep = t->keep_stage;
    }
    TH_CHECK_HIP(hipSetDevice(t->ctx->p.device));
    hipStream_t s = t->ctx->stream;
    const float scale = 1.0f / (1.0f - P_DROP);
    const uint8_t* keep = d_keep;
    if (!keep) {
        // the three planes behind the pools are one draw; the head's plane comes from another stream of the same counter hash, as for v100 and v110
        t_masks(s, t->keep, (size_t)n * t->keep_off[3], t->p.seed, (uint64_t)t->step, P_DROP);
        t_masks(s, t->keep + (size_t)n * t->keep_off[3], (size_t)n * HID, t->p.seed ^ 0xD1B54A32D192ED03ull, (uint64_t)t->step, P_DROP);
        keep = t->keep;
    }
    t_check_targets(s, targets, n, t->classes, t->bad_target, 0);
    trainer_forward(t, s, x, targets, n, keep, scale, true);
    // ---- backward
    tarch_head_grads(s, t->dl, t->hd, t->dh, n, t->classes, t->grad(S_F2W), t->grad(S_F2B), t->grad(S_F1B));
    tany_fc1_wgrad(s, t->geom, n, t->L[2].a, t->dh, t->grad(S_F1W));
    t_loss(s, t->loss, t->correct, n, t->out2);
    tany_fc1_dgrad(s, t->geom, n, t->dh, t->param(S_F1W), t->L[2].da);
    for (int i = 2; i >= 0; --i) block_backward(t, s, t->L[i], n, keep, scale);
    tany_wgrad1(s, t->geom, n, x, t->L[0].z, t->part1);
    t_reduce(s, t->part1, n * t->geom.wg1_tiles, t->CH * T2 * 16, t->grad(K_W));
    // ---- optimizer
    t->step += 1;
    {
        uint32_t lo[3], hi[3];                                   // running statistics are buffers: mean and variance of a BatchNorm lie side by side
        for (int i = 0; i < 3; ++i) { lo[i] = (uint32_t)t->off[6 * i + K_RM]; hi[i] = (uint32_t)(t->off[6 * i + K_RV] + t->isz[6 * i + K_RV]); }
        t_adam(s, t->P, t->G, t->M, t->V, t->total, lo, hi, 3, t->p.lr, t->p.beta1, t->p.beta2, t->p.eps, t->step, t->bad_target);
    }
    TH_CHECK_HIP(hipGetLastError());
    if (h_loss || h_correct) { if (const int rc = fetch_loss(t, s, h_loss, h_correct)) return rc; }
    if (host) TH_CHECK_HIP(hipStreamSynchronize(s));             // the caller's buffers may go away
    return TREXHIP_OK;
}

int cat_trainer_eval(CatTrainer* t, bool host, const float* x, const int32_t* targets, int n, float* h_loss, int32_t* h_correct) {
    if (host) {
        if (const int rc = stage(t, "trexhip_train_eval", x, targets, n, nullptr)) return rc;
        x = t->x_stage; targets = t->y_stage;
    }
    TH_CHECK_HIP(hipSetDevice(t->ctx->p.device));
    hipStream_t s = t->ctx->stream;
    TH_CHECK_HIP(hipMemsetAsync(t->keep, 1, (size_t)n * t->keep_row, s));                 // nothing dropped
    t_check_targets(s, targets, n, t->classes, t->bad_target, 1);
    trainer_forward(t, s, x, targets, n, t->keep, 1.f, false);
    t_loss(s, t->loss, t->correct, n, t->out2);
    TH_CHECK_HIP(hipGetLastError());
    return fetch_loss(t, s, h_loss, h_correct);
}

int cat_trainer_predict(CatTrainer* t, const uint8_t* d_crops, int n, float* d_probs) {
    trexhip_ctx* ctx = t->ctx;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    TH_CHECK_HIP(hipMemsetAsync(t->keep, 1, (size_t)std::min(n, t->max_n) * t->keep_row, s));       // nothing dropped
    for (int at = 0; at < n; at += t->max_n) {
        const int m = std::min(t->max_n, n - at);
        const int rc = trexhip_augment_device(ctx, nullptr, d_crops + (size_t)at * t->H * t->W * t->CH, nullptr, m, nullptr, m, t->W, t->H, t->CH, nullptr, 0, 0, t->x_stage, nullptr);
        if (rc != TREXHIP_OK) return rc;
        trainer_forward(t, s, t->x_stage, nullptr, m, t->keep, 1.f, false, d_probs + (size_t)at * t->classes);
    }
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

int cat_trainer_read(CatTrainer* t, int32_t tensor, int32_t kind, float* out, size_t count) {
    if (!out || tensor < 0 || tensor >= S_COUNT || kind < 0 || kind > 3) { set_error("trexhip_trainer_read: bad argument"); return TREXHIP_E_INVALID; }
    const int slot = ORDER[tensor];
    if (count != t->cnt[slot]) { set_error("trexhip_trainer_read: count does not match the tensor"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(t->ctx->p.device));
    TH_CHECK_HIP(hipStreamSynchronize(t->ctx->stream));
    { const int rc = check_targets(t); if (rc != TREXHIP_OK) return rc; }
    const float* src = kind == 0 ? t->P : kind == 1 ? t->G : kind == 2 ? t->M : t->V;
    std::vector<float> tmp(t->isz[slot]);
    TH_CHECK_HIP(hipMemcpy(tmp.data(), src + t->off[slot], tmp.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < count; ++i) out[i] = tmp[to_internal(slot, i, t->CH, (size_t)t->geom.P)];
    return TREXHIP_OK;
}

int cat_trainer_export(CatTrainer* t, void* blob, size_t capacity, size_t* bytes) {
    const size_t need = category_blob_bytes(t->classes, t->CH, t->W, t->H);
    if (bytes) *bytes = need;
    if (capacity < need) { set_error("trexhip_trainer_export: buffer too small (the bytes of the blob the trainer was created from)"); return TREXHIP_E_CAPACITY; }
    write_category_blob_header(blob, t->classes, t->W, t->H, t->CH);
    float* dst = reinterpret_cast<float*>(static_cast<char*>(blob) + 32);
    for (int k = 0; k < S_COUNT; ++k) {
        const size_t cnt = t->cnt[ORDER[k]];
        if (const int rc = cat_trainer_read(t, k, 0, dst, cnt)) return rc;
        dst += cnt;
    }
    return TREXHIP_OK;
}

}  // namespace trexhip
