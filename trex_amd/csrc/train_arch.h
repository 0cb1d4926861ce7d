// train_arch.h -- the trainer of the identity networks v100 and v110 (train_arch.hip) as train.hip's entry points call it: every
// trexhip_trainer_* / trexhip_train_* call of a trainer created from such a blob lands in the function of the same name here.  Not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
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

}  // namespace trexhip
