// train_arch.h -- the trainer of the one-stream chain (train_arch.hip: v100, v110, the category network) as trexhip_trainer_create reaches it.  Every
// other call of such a trainer goes through TrainerCore (train_host.h).  Not part of the ABI.
#pragma once
#include "train_host.h"

namespace trexhip {

// blob: a 'TRXC' blob (parse_category_blob) or an identity blob whose header names v100 or v110 (parse_arch_blob)
int chain_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, TrainerCore** out);

}  // namespace trexhip
