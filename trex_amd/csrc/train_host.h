// train_host.h -- what every trainer holds and does on the host (train_host.hip), stated once: the state behind a trexhip_trainer handle, the
// staging of a host batch, the refusals, evaluation, the chunked prediction, read, export, the create-time upload, the Adam call and the teardown.
// A concrete trainer -- Trainer (train.hip: V118_3) or ChainTrainer (train_arch.hip: v100, v110, the category network) -- derives from
// TrainerCore and supplies its chain through the virtual functions below.  The second half declares the launches of train.hip's size-independent
// kernels as the core and the other chain call them.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "internal.h"
#include "train_tensors.h"

namespace trexhip {

struct TrainerCore {
    trexhip_ctx* ctx = nullptr;
    int version = 0, classes = 0, CH = 1, W = 0, H = 0, max_n = 0;
    trexhip_train_params p{};
    int64_t step = 0;
    TrainTensors tt{};                     // off, cnt, isz, order, n_tensors, total; keep_off, keep_row; the buffers Adam skips
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;      // parameters, gradients, Adam's moments: one layout (tt.off)
    float *loss = nullptr, *out2 = nullptr;
    int32_t *correct = nullptr, *bad_target = nullptr;                 // bad_target: steps / evaluations the device refused, sticky until read
    uint8_t *keep = nullptr, *keep_stage = nullptr;
    float* x_stage = nullptr;              // host-pointer entry points: inputs, targets and injected masks staged here
    int32_t* y_stage = nullptr;
    Mem mem;                               // every device buffer of the trainer

    float* param(int slot) const { return P + tt.off[slot]; }
    float* grad(int slot) const { return G + tt.off[slot]; }

    // ---- what a concrete trainer supplies
    virtual ~TrainerCore() { mem.free_all(); }                        // its own teardown extras in its destructor, which runs first
    // a step refused before anything is staged or queued (v110: n < 2); sets the error
    virtual int refuse_step(const char* who, int n) { (void)who; (void)n; return TREXHIP_OK; }
    // the masks of a training step: `injected` (device) or a draw into `keep`; returns the masks the step reads
    virtual const uint8_t* begin_step(hipStream_t s, int n, const uint8_t* injected) = 0;
    // x -> per-sample loss / arg-max and the head's gradients.  train: batch statistics and dropout; else running statistics, `keep` is all ones.
    // probs: a prediction, the softmax rows and nothing else
    virtual void forward(hipStream_t s, const float* x, const int32_t* targets, int n, const uint8_t* keep, bool train, float* probs) = 0;
    // everything between forward and Adam: every gradient into G, the loss sum into out2
    virtual void backward(hipStream_t s, const float* x, int n, const uint8_t* keep) = 0;
    virtual size_t blob_bytes() const = 0;
    virtual void write_blob_header(void* blob) const = 0;

    // ---- what all of them do (train_host.hip)
    // the rest of a create: P / G / M / V and the core's own buffers, the blob's tensors (src[slot], torch's layout) uploaded in the kernels' layout
    int init_state(const float* const* src, const char* who);
    int check_targets();
    int fetch_loss(hipStream_t s, float* h_loss, int32_t* h_correct);
    int stage(const char* who, const float* inputs, const int32_t* targets, int n, const uint8_t* keep_masks);
    void adam(hipStream_t s);
    // device pointers (host = false) or host pointers staged through the trainer's buffers (host = true); 1 <= n <= max_batch was checked
    int train_step(bool host, const float* x, const int32_t* targets, int n, const uint8_t* keep_masks, float* h_loss, int32_t* h_correct);
    int eval(bool host, const float* x, const int32_t* targets, int n, float* h_loss, int32_t* h_correct);
    int predict(const uint8_t* d_crops, int n, float* d_probs);
    int read(int32_t tensor, int32_t kind, float* out, size_t count);
    int export_blob(void* blob, size_t capacity, size_t* bytes);
};

// what trexhip_trainer_create asks of its parameters, whatever the network: a chain trainer judges them before it parses its blob, V118_3 behind
// its parser
int check_train_params(const trexhip_train_params* p);
// train.hip: a V118_3 blob (parse_weight_blob)
int v118_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, TrainerCore** out);

// ---- the launches of train.hip's size-independent kernels.  Everything is queued on the given stream, nothing synchronises
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
void t_wgrad_reduce(hipStream_t s, const float* part, int shares, int CI, int CO, int CIC, float* g, int taps);
// k_t_reduce: out[count] = sum of nparts parts, fixed order
void t_reduce(hipStream_t s, const float* part, int nparts, int count, float* out);
// k_t_repack_bwd: the data gradient's flipped + transposed weights
void t_repack_bwd(hipStream_t s, const float* wf, int CI, int CO, int CIC, int COP, int CICB, float* wb, int taps);
// k_t_adam over [0, total) but the `nskip` (at most 6) ranges [lo, hi) of buffers
void t_adam(hipStream_t s, float* P, const float* G, float* M, float* V, size_t total, const uint32_t* skip_lo, const uint32_t* skip_hi, int nskip, double lr,
            double beta1, double beta2, float eps, int64_t step, const int32_t* refused);
void t_masks(hipStream_t s, uint8_t* keep, size_t count, uint64_t seed, uint64_t step, float p_drop);
void t_check_targets(hipStream_t s, const int32_t* targets, int n, int classes, int32_t* refused, int eval);
void t_loss(hipStream_t s, const float* loss, const int32_t* correct, int n, float* out2);

}  // namespace trexhip
