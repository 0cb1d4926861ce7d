// train_shared.h -- the launches of train.hip's size-independent kernels (reductions, the optimizer, the masks, the target check, the loss sum) as
// another chain calls them: train_arch.hip (v100, v110) and train_cat.hip (the category network) run them unchanged.  Everything is queued on the
// given stream, nothing synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace trexhip {

constexpr int T_RED_BLOCKS = 256, T_BWD_BLOCKS = 1024;     // grids of the reduction kernels: partials are [block][planes][C] doubles

// k_t_bn_stats<C>: per-channel sum and sum of squares of d[rows][C] (C = 16, 64, 128) -> partial[T_RED_BLOCKS][2][C]
void t_bn_stats(hipStream_t s, int C, const float* d, size_t rows, double* partial);
// k_t_red_finalize<FIN_BN_STATS>: mean, invstd (biased variance) and the running statistics (unbiased variance, momentum; left alone when *refused)
void t_fin_bn_stats(hipStream_t s, const double* partial, int nblocks, int C, double count, float momentum, float* mean, float* invstd, float* run_mean,
                    float* run_var, const int32_t* refused);
// k_t_red_finalize<FIN_BN_BWD>: sums[2][C] = sum dy, sum dy x-hat; d_gamma = the second, d_beta = the first
void t_fin_bn_bwd(hipStream_t s, const double* partial, int nblocks, int C, float* sums, float* d_gamma, float* d_beta);
// k_t_red_finalize<FIN_BIAS>: d_bias[C] = the column sums
void t_fin_bias(hipStream_t s, const double* partial, int nblocks, int C, float* d_bias);
// k_t_bn_from_running: eval mode's mean and invstd
void t_bn_from_running(hipStream_t s, const float* run_mean, const float* run_var, int C, float* mean, float* invstd);
// k_t_wgrad_reduce: part[shares][T][CI][CO] -> g in the parameter layout [CI / CIC][T][CIC][CO], T = taps^2
void t_wgrad_reduce(hipStream_t s, const float* part, int shares, int CI, int CO, int CIC, float* g, int taps = 5);
// k_t_reduce: out[count] = sum of nparts parts, fixed order
void t_reduce(hipStream_t s, const float* part, int nparts, int count, float* out);
// k_t_repack_bwd: the data gradient's flipped + transposed weights
void t_repack_bwd(hipStream_t s, const float* wf, int CI, int CO, int CIC, int COP, int CICB, float* wb, int taps = 5);
// k_t_adam over [0, total) but the `nskip` (at most 6) ranges [lo, hi) of buffers
void t_adam(hipStream_t s, float* P, const float* G, float* M, float* V, size_t total, const uint32_t* skip_lo, const uint32_t* skip_hi, int nskip, double lr,
            double beta1, double beta2, float eps, int64_t step, const int32_t* refused);
void t_masks(hipStream_t s, uint8_t* keep, size_t count, uint64_t seed, uint64_t step, float p_drop);
void t_check_targets(hipStream_t s, const int32_t* targets, int n, int classes, int32_t* refused, int eval);
void t_loss(hipStream_t s, const float* loss, const int32_t* correct, int n, float* out2);

}  // namespace trexhip
