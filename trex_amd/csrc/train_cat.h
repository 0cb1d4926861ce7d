// train_cat.h -- the trainer of the category network (train_cat.hip) as train.hip's entry points call it: every trexhip_trainer_* / trexhip_train_*
// call of a trainer created from a 'TRXC' blob lands in the function of the same name here.  Not part of the ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/trexhip.h"

namespace trexhip {

struct CatTrainer;

// blob: parsed by parse_category_blob (the parser of trexhip_categorize_load_weights).  p has passed trexhip_trainer_create's checks
int cat_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, CatTrainer** out);
void cat_trainer_destroy(CatTrainer* t);
void cat_trainer_set_lr(CatTrainer* t, float lr);
int64_t cat_trainer_steps(const CatTrainer* t);
void cat_trainer_info(const CatTrainer* t, int32_t* width, int32_t* height, int32_t* max_batch);
size_t cat_trainer_keep_mask_bytes(const CatTrainer* t, int n);      // n * (h1 w1 16 + h2 w2 64 + h3 w3 100 + 100), the pooled planes by successive floors
// device pointers (host = false) or host pointers staged through the trainer's buffers (host = true); 1 <= n <= max_batch was checked
int cat_trainer_step(CatTrainer* t, bool host, const float* inputs, const int32_t* targets, int n, const uint8_t* keep_masks, float* loss, int32_t* correct);
int cat_trainer_eval(CatTrainer* t, bool host, const float* inputs, const int32_t* targets, int n, float* loss, int32_t* correct);
int cat_trainer_predict(CatTrainer* t, const uint8_t* d_crops, int n, float* d_probs);
int cat_trainer_read(CatTrainer* t, int32_t tensor, int32_t kind, float* out, size_t count);
int cat_trainer_export(CatTrainer* t, void* blob, size_t capacity, size_t* bytes);

}  // namespace trexhip
