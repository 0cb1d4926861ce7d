// train_host.hip -- the host side every trainer shares (train_host.h) and the trexhip_trainer_* / trexhip_train_* entry points.  This file holds no
// kernel: the chain of a step is the concrete trainer's (train.hip: V118_3; train_arch.hip: v100, v110, the category network), reached through
// TrainerCore's virtual functions, and the few launches queued here (the target check, the loss sum, Adam) are train.hip's kernels.
// The order in which a batch call refuses: the handle, its pointers and n (check_batch), the trainer's own refusal (v110: n >= 2), the targets'
// range on the host (host pointers only), then whatever the device finds.
#include "internal.h"
#include "cnn_weights.h"
#include "train_host.h"
#include "train_arch.h"
#include <algorithm>
#include <string>
#include <vector>

namespace trexhip {

int TrainerCore::init_state(const float* const* src, const char* who) {
    const size_t n = (size_t)max_n, at = tt.total;
    int rc = TREXHIP_OK;
#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)
    TRY(mem.device(&P, at, who)); TRY(mem.device(&G, at, who)); TRY(mem.device(&M, at, who)); TRY(mem.device(&V, at, who));
    TRY(mem.device(&loss, n, who)); TRY(mem.device(&correct, n, who)); TRY(mem.device(&out2, 2, who)); TRY(mem.device(&bad_target, 2, who));
    TRY(mem.device(&keep, n * tt.keep_row, who)); TRY(mem.device(&keep_stage, n * tt.keep_row, who));
    TRY(mem.device(&x_stage, n * H * W * CH, who)); TRY(mem.device(&y_stage, n, who));
#undef TRY
    if (rc != TREXHIP_OK) return rc;
    std::vector<float> host(at, 0.f);
    for (int k = 0; k < tt.n_slots; ++k)
        for (size_t i = 0; i < tt.cnt[k]; ++i) host[tt.off[k] + tt.to_internal(k, i)] = src[k][i];
    bool ok = hipMemcpy(P, host.data(), at * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(bad_target, 0, 8) == hipSuccess;
    ok = ok && hipMemset(G, 0, at * 4) == hipSuccess && hipMemset(M, 0, at * 4) == hipSuccess && hipMemset(V, 0, at * 4) == hipSuccess;
    if (!ok) { set_error(std::string(who) + ": upload failed"); return TREXHIP_E_DEVICE; }
    return TREXHIP_OK;
}

// steps with a target outside 0..classes-1 were refused on the device (k_t_check_targets) and have changed nothing: report them at the next
// synchronising call, take them back out of the step count (Adam's bias correction, the dropout counter) and go on
int TrainerCore::check_targets() {
    int32_t bad[2] = {0, 0};
    TH_CHECK_HIP(hipMemcpy(bad, bad_target, 8, hipMemcpyDeviceToHost));
    if (bad[0] || bad[1]) {
        TH_CHECK_HIP(hipMemset(bad_target, 0, 8));
        if (bad[0]) step -= bad[0];
        set_error(bad[0] ? std::string("training step: a target class index was outside 0..classes-1; that step (and the ") + std::to_string(bad[0] - 1) +
                               " queued behind it) was refused, parameters, moments and running statistics are unchanged"
                         : std::string("evaluation batch: a target class index was outside 0..classes-1"));
        return TREXHIP_E_INVALID;
    }
    return TREXHIP_OK;
}

// the loss and the correct count of the batch just queued, to the host (synchronises), and what the device refused
int TrainerCore::fetch_loss(hipStream_t s, float* h_loss, int32_t* h_correct) {
    float two[2];
    TH_CHECK_HIP(hipMemcpyAsync(two, out2, sizeof(two), hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    if (h_loss) *h_loss = two[0];
    if (h_correct) *h_correct = (int32_t)two[1];
    return check_targets();
}

// the host-pointer entry points: the targets' range before anything is uploaded (visual_recognition_torch.py:1112), then the batch into the
// staging buffers on the context's stream
int TrainerCore::stage(const char* who, const float* inputs, const int32_t* targets, int n, const uint8_t* keep_masks) {
    for (int i = 0; i < n; ++i)
        if (targets[i] < 0 || targets[i] >= classes) { set_error(std::string(who) + ": target class out of range"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    TH_CHECK_HIP(hipMemcpyAsync(x_stage, inputs, (size_t)n * H * W * CH * sizeof(float), hipMemcpyHostToDevice, s));
    TH_CHECK_HIP(hipMemcpyAsync(y_stage, targets, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (keep_masks) TH_CHECK_HIP(hipMemcpyAsync(keep_stage, keep_masks, (size_t)n * tt.keep_row, hipMemcpyHostToDevice, s));
    return TREXHIP_OK;
}

// running statistics are buffers: Adam skips them.  Slots side by side (the mean and the variance of a BatchNorm) are one range
void TrainerCore::adam(hipStream_t s) {
    uint32_t lo[8], hi[8];
    int k = 0;
    for (int i = 0; i < tt.n_buffers; ++i) {
        const int b = tt.buffers[i];
        if (i && tt.buffers[i - 1] == b - 1) { hi[k - 1] = (uint32_t)(tt.off[b] + tt.isz[b]); continue; }
        lo[k] = (uint32_t)tt.off[b]; hi[k] = (uint32_t)(tt.off[b] + tt.isz[b]); ++k;
    }
    t_adam(s, P, G, M, V, tt.total, lo, hi, k, p.lr, p.beta1, p.beta2, p.eps, step, bad_target);
}

int TrainerCore::train_step(bool host, const float* x, const int32_t* targets, int n, const uint8_t* keep_masks, float* h_loss, int32_t* h_correct) {
    const char* who = host ? "trexhip_train_step" : "trexhip_train_step_device";
    if (const int rc = refuse_step(who, n)) return rc;
    if (host) {
        if (const int rc = stage(who, x, targets, n, keep_masks)) return rc;
        x = x_stage; targets = y_stage;
        if (keep_masks) keep_masks = keep_stage;
    }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    const uint8_t* kp = begin_step(s, n, keep_masks);
    t_check_targets(s, targets, n, classes, bad_target, 0);
    forward(s, x, targets, n, kp, true, nullptr);
    backward(s, x, n, kp);
    step += 1;
    adam(s);
    TH_CHECK_HIP(hipGetLastError());
    if (h_loss || h_correct) { if (const int rc = fetch_loss(s, h_loss, h_correct)) return rc; }
    if (host) TH_CHECK_HIP(hipStreamSynchronize(s));             // the caller's buffers may go away
    return TREXHIP_OK;
}

// model.eval() forward + mean cross entropy + arg-max count of one validation batch (train(), visual_recognition_torch.py:1171-1190); changes
// nothing in the trainer
int TrainerCore::eval(bool host, const float* x, const int32_t* targets, int n, float* h_loss, int32_t* h_correct) {
    if (host) {
        if (const int rc = stage("trexhip_train_eval", x, targets, n, nullptr)) return rc;
        x = x_stage; targets = y_stage;
    }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    TH_CHECK_HIP(hipMemsetAsync(keep, 1, (size_t)n * tt.keep_row, s));                 // nothing dropped
    t_check_targets(s, targets, n, classes, bad_target, 1);
    forward(s, x, targets, n, keep, false, nullptr);
    t_loss(s, loss, correct, n, out2);
    TH_CHECK_HIP(hipGetLastError());
    return fetch_loss(s, h_loss, h_correct);
}

// softmax rows of any number of uint8 crops from the weights as they stand (predict_numpy in model.eval(), visual_recognition_torch.py:406-451):
// chunks of at most max_batch through the trainer's own buffers -- bytes -> float32 in x_stage (k_augment's plain path), the eval forward -- all
// on the context's stream, no synchronisation.  Parameters, moments, running statistics and the step count stay as they are
int TrainerCore::predict(const uint8_t* d_crops, int n, float* d_probs) {
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    TH_CHECK_HIP(hipMemsetAsync(keep, 1, (size_t)std::min(n, max_n) * tt.keep_row, s));       // nothing dropped
    for (int at = 0; at < n; at += max_n) {
        const int m = std::min(max_n, n - at);
        const int rc = trexhip_augment_device(ctx, nullptr, d_crops + (size_t)at * H * W * CH, nullptr, m, nullptr, m, W, H, CH, nullptr, 0, 0, x_stage, nullptr);
        if (rc != TREXHIP_OK) return rc;
        forward(s, x_stage, nullptr, m, keep, false, d_probs + (size_t)at * classes);
    }
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

int TrainerCore::read(int32_t tensor, int32_t kind, float* out, size_t count) {
    if (!out || tensor < 0 || tensor >= tt.n_tensors || kind < 0 || kind > 3) { set_error("trexhip_trainer_read: bad argument"); return TREXHIP_E_INVALID; }
    const int slot = tt.order[tensor];
    if (count != tt.cnt[slot]) { set_error("trexhip_trainer_read: count does not match the tensor"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    { const int rc = check_targets(); if (rc != TREXHIP_OK) return rc; }
    const float* src = kind == 0 ? P : kind == 1 ? G : kind == 2 ? M : V;
    std::vector<float> tmp(tt.isz[slot]);
    TH_CHECK_HIP(hipMemcpy(tmp.data(), src + tt.off[slot], tmp.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < count; ++i) out[i] = tmp[tt.to_internal(slot, i)];
    return TREXHIP_OK;
}

int TrainerCore::export_blob(void* blob, size_t capacity, size_t* bytes) {
    const size_t need = blob_bytes();
    if (bytes) *bytes = need;
    if (capacity < need) { set_error("trexhip_trainer_export: buffer too small (the bytes of the blob the trainer was created from)"); return TREXHIP_E_CAPACITY; }
    write_blob_header(blob);
    float* dst = reinterpret_cast<float*>(static_cast<char*>(blob) + 32);
    for (int k = 0; k < tt.n_tensors; ++k) {
        const size_t cnt = tt.cnt[tt.order[k]];
        if (const int rc = read(k, 0, dst, cnt)) return rc;
        dst += cnt;
    }
    return TREXHIP_OK;
}

// what trexhip_trainer_create asks of its parameters, whatever the network
int check_train_params(const trexhip_train_params* p) {
    if (p->max_batch < 1 || p->max_batch > 4096) { set_error("trexhip_trainer_create: max_batch must be 1..4096"); return TREXHIP_E_INVALID; }
    if (p->precision != 0 && p->precision != 1) { set_error("trexhip_trainer_create: precision must be 0 (fp16 two-piece split convolutions) or 1 (exact fp32 MFMA)"); return TREXHIP_E_INVALID; }
    if (!(p->lr > 0.f) || !(p->beta1 >= 0.f && p->beta1 < 1.f) || !(p->beta2 >= 0.f && p->beta2 < 1.f) || !(p->eps > 0.f) ||
        !(p->dropout >= 0.f && p->dropout < 1.f) || !(p->bn_momentum >= 0.f && p->bn_momentum <= 1.f)) {
        set_error("trexhip_trainer_create: lr > 0, 0 <= beta < 1, eps > 0, 0 <= dropout < 1, 0 <= bn_momentum <= 1 are required");
        return TREXHIP_E_INVALID;
    }
    return TREXHIP_OK;
}

}  // namespace trexhip

struct trexhip_trainer { trexhip::TrainerCore* core; };

extern "C" {

using namespace trexhip;

// The blob chooses the trainer: a category blob ('TRXC') or one whose header names v100 / v110 trains on the one-stream chain (train_arch.hip), every
// other identity blob is V118_3's business (train.hip: its parser refuses what does not train)
int trexhip_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, trexhip_trainer** out) {
    if (!ctx || !blob || !p || !out) { set_error("trexhip_trainer_create: null argument"); return TREXHIP_E_INVALID; }
    *out = nullptr;
    const int arch = blob_arch_id(blob, bytes);
    const bool chain = blob_is_category(blob, bytes) || arch == TREXHIP_NET_V100 || arch == TREXHIP_NET_V110;
    TrainerCore* core = nullptr;
    if (const int rc = chain ? chain_trainer_create(ctx, blob, bytes, p, &core) : v118_trainer_create(ctx, blob, bytes, p, &core)) return rc;
    *out = new trexhip_trainer{core};
    return TREXHIP_OK;
}

void trexhip_trainer_destroy(trexhip_trainer* h) {
    if (!h) return;
    (void)hipSetDevice(h->core->ctx->p.device);
    (void)hipStreamSynchronize(h->core->ctx->stream);
    delete h->core;
    delete h;
}

int trexhip_trainer_set_lr(trexhip_trainer* h, float lr) {
    if (!h || !(lr > 0.f)) { set_error("trexhip_trainer_set_lr: a trainer and lr > 0 are required"); return TREXHIP_E_INVALID; }
    h->core->p.lr = lr;
    return TREXHIP_OK;
}

int64_t trexhip_trainer_steps(trexhip_trainer* h) { return h ? h->core->step : -1; }

int trexhip_trainer_image_size(trexhip_trainer* h, int32_t* width, int32_t* height) {
    if (!h || !width || !height) { set_error("trexhip_trainer_image_size: null argument"); return TREXHIP_E_INVALID; }
    *width = h->core->W; *height = h->core->H;
    return TREXHIP_OK;
}

int trexhip_trainer_version(trexhip_trainer* h, int32_t* version) {
    if (!h || !version) { set_error("trexhip_trainer_version: null argument"); return TREXHIP_E_INVALID; }
    *version = h->core->version;
    return TREXHIP_OK;
}

size_t trexhip_trainer_keep_mask_bytes(trexhip_trainer* h, int32_t n) { return !h || n < 0 ? 0 : (size_t)n * h->core->tt.keep_row; }

// what every batch entry point checks first: the handle, its two pointers, 1 <= n <= max_batch (any_n: no upper bound, the call chunks)
static int check_batch(const char* who, const trexhip_trainer* h, const void* a, const void* b, int n, bool any_n = false) {
    if (!h || !a || !b) { set_error(std::string(who) + ": null argument"); return TREXHIP_E_INVALID; }
    if (n < 1 || (!any_n && n > h->core->max_n)) { set_error(std::string(who) + (any_n ? ": n must be at least 1" : ": n must be 1..max_batch")); return TREXHIP_E_INVALID; }
    return TREXHIP_OK;
}

int trexhip_train_step_device(trexhip_trainer* h, const float* d_inputs, const int32_t* d_targets, int32_t n, const uint8_t* d_keep_masks, float* loss,
                              int32_t* correct) {
    if (const int rc = check_batch("trexhip_train_step_device", h, d_inputs, d_targets, n)) return rc;
    return h->core->train_step(false, d_inputs, d_targets, n, d_keep_masks, loss, correct);
}

int trexhip_train_step(trexhip_trainer* h, const float* inputs, const int32_t* targets, int32_t n, const uint8_t* keep_masks, float* loss, int32_t* correct) {
    if (const int rc = check_batch("trexhip_train_step", h, inputs, targets, n)) return rc;
    return h->core->train_step(true, inputs, targets, n, keep_masks, loss, correct);
}

int trexhip_train_eval_device(trexhip_trainer* h, const float* d_inputs, const int32_t* d_targets, int32_t n, float* loss, int32_t* correct) {
    if (const int rc = check_batch("trexhip_train_eval_device", h, d_inputs, d_targets, n)) return rc;
    return h->core->eval(false, d_inputs, d_targets, n, loss, correct);
}

int trexhip_train_eval(trexhip_trainer* h, const float* inputs, const int32_t* targets, int32_t n, float* loss, int32_t* correct) {
    if (const int rc = check_batch("trexhip_train_eval", h, inputs, targets, n)) return rc;
    return h->core->eval(true, inputs, targets, n, loss, correct);
}

int trexhip_train_predict_device(trexhip_trainer* h, const uint8_t* d_crops, int32_t n, float* d_probs) {
    if (const int rc = check_batch("trexhip_train_predict_device", h, d_crops, d_probs, n, true)) return rc;
    return h->core->predict(d_crops, n, d_probs);
}

int trexhip_trainer_read(trexhip_trainer* h, int32_t tensor, int32_t kind, float* out, size_t count) {
    if (!h) { set_error("trexhip_trainer_read: bad argument"); return TREXHIP_E_INVALID; }
    return h->core->read(tensor, kind, out, count);
}

int trexhip_trainer_export(trexhip_trainer* h, void* blob, size_t capacity, size_t* bytes) {
    if (!h || !blob) { set_error("trexhip_trainer_export: null argument"); return TREXHIP_E_INVALID; }
    return h->core->export_blob(blob, capacity, bytes);
}

}  // extern "C"
