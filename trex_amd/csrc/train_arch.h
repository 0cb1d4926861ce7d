// train_arch.h -- the trainer of the identity networks v100 and v110 (train_arch.hip) as train.hip's entry points call it: every
// trexhip_trainer_* / trexhip_train_* call of a trainer created from such a blob lands in the function of the same name here.  Not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "../../include/trexhip.h"

namespace trexhip {

struct ArchTrainer;

// blob: parsed by parse_arch_blob (the parser of trexhip_load_weights); v100 and v110 only.  p has passed trexhip_trainer_create's checks
int arch_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, ArchTrainer** out);
void arch_trainer_destroy(ArchTrainer* t);
void arch_trainer_set_lr(ArchTrainer* t, float lr);
int64_t arch_trainer_steps(const ArchTrainer* t);
void arch_trainer_info(const ArchTrainer* t, int32_t* width, int32_t* height, int32_t* version, int32_t* max_batch);
// device pointers (host = false) or host pointers staged through the trainer's buffers (host = true); 1 <= n <= max_batch was checked
int arch_trainer_step(ArchTrainer* t, bool host, const float* inputs, const int32_t* targets, int n, const uint8_t* keep_masks, float* loss, int32_t* correct);
int arch_trainer_eval(ArchTrainer* t, bool host, const float* inputs, const int32_t* targets, int n, float* loss, int32_t* correct);
int arch_trainer_predict(ArchTrainer* t, const uint8_t* d_crops, int n, float* d_probs);
int arch_trainer_read(ArchTrainer* t, int32_t tensor, int32_t kind, float* out, size_t count);
int arch_trainer_export(ArchTrainer* t, void* blob, size_t capacity, size_t* bytes);
size_t arch_trainer_keep_mask_bytes(int n);       // n * (16 + 64 + 100 + 100)

// v100's head for another chain (the category network, train_cat.hip): hsum [n][100] = fc1 without its bias -> + b1, ReLU, element-wise dropout
// (keep [n][100]), fc2, softmax cross entropy; hd = the dropped activations, dl = d(logits), dh = d(fc1 output).  probs != null: softmax rows only
void tarch_head_plain(hipStream_t s, const float* hsum, int n, const float* b1, const uint8_t* keep, float scale, const float* w2, const float* b2, const int32_t* targets,
                      int classes, float* hd, float* dl, float* dh, float* loss, int32_t* correct, float* probs);
// fc2 weight / bias and fc1 bias gradients, the samples in order
void tarch_head_grads(hipStream_t s, const float* dl, const float* hd, const float* dh, int n, int classes, float* g_w2, float* g_b2, float* g_b1);

}  // namespace trexhip
