// train.hip -- one optimizer step of the identity network V118_3 on gfx950, fp32.
//
// Replaces the body of train()'s batch loop
//   Application/src/tracker/python/visual_recognition_torch.py:1137-1158
//       outputs = model(inputs); loss = CrossEntropyLoss(outputs, targets); loss.backward(); optimizer.step(); zero_grad()
//   (criterion / Adam(lr) :1420-1421; autocast + GradScaler are enabled for device == 'cuda' only, :1066-1072 -- fp32 is the
//   reference's own arithmetic everywhere else and the parity bar here)
// for the network visual_identification_network_torch.py:184-258 in TRAINING mode:
//   [conv5x5 'same' -> BatchNorm2d (batch statistics; running statistics updated, momentum 0.1) -> ReLU -> MaxPool2 ->
//    Dropout2d(0.05)] x3 -> flatten (NCHW order) -> fc1 -> LayerNorm(100) -> ReLU -> Dropout(0.05) -> fc2 -> cross entropy (mean).
// Inputs are what TRexImageDataset yields (:158-188): NHWC float32 in [0, 255], integer class labels.
//
// Data (all NHWC fp32 in HBM, sized for max_batch at creation): z_i = raw convolution outputs (kept for the backward pass, turned
// into dz_i in place), a_i = pooled + dropped activations, da_i = their gradients.  Parameters, gradients and the two Adam moments are
// four flat arrays with one layout (the kernels' layouts, not torch's: conv [ci chunk][tap][ci][co], fc1 [hw][c][o]), so the
// optimizer is one element-wise launch; import / export / read permute on the host.
// Kernels: convolutions and data gradients = k_conv5 (conv_f32.h, fp32 MFMA, raw epilogue; the data gradient is the same kernel on
// flipped + transposed weights); weight gradients = k_t_wgrad (fp32 MFMA, operands straight from L2: one MFMA k-step = two pixels,
// A = activations at the tap's shift, B = dz); batch-norm statistics and their backward sums in double; everything else VALU.
// Every reduction has a fixed order: two runs of a step give identical bits.
// Host side (below the kernels): `Trainer` derives from TrainerCore (train_host.h), which holds what every trainer holds and does -- the tensors
// (train_tensors.h), P / G / M / V, staging, the refusals, evaluation, prediction, read, export, the Adam call and the walk of a step -- and
// supplies V118_3's chain: begin_step (the fork, the masks), forward, backward.  Each of the three blocks is one `Layer` -- shape, tensor ids,
// buffers, and the kernel instances of the trainer's precision bound to their LDS sizes -- filled once in v118_trainer_create; the forward
// pass, block_backward and trainer_attrs walk that table.
// The convolutions of this file -- conv1 with its fused column sums, conv2 / conv3 in their three roles, conv1's weight gradient -- are the
// 80x80 chain's: tilings, a summation order and the fp16 two-piece path of their own.  A blob of any other individual_image_size (8..256 each
// way) trains on the convolutions of train_any.hip (exact fp32, geometry in train_geom.h): the same walk, with `Trainer::any` choosing the
// launch where the algorithm differs -- those convolutions, the head's plane count, the partial-buffer sizes.  What merely follows the plane's
// size -- BN + ReLU + pool + dropout and its way back, fc1 and its two gradients -- is train_any.hip's k_tany_ kernels at every size, 80x80
// included; the head, Adam, the masks, the target check, the loss and the reductions do not depend on the size.
// A v100, v110 or category ('TRXC') blob gives a ChainTrainer (train_arch.hip) instead: trexhip_trainer_create (train_host.hip) chooses by the
// blob, and that chain and the core launch this file's size-independent kernels through the t_* functions declared in train_host.h.
#include "internal.h"
#include "conv_f32.h"
#include "cnn_weights.h"
#include "train_dev.h"
#include "train_any.h"
#include "train_host.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <string>
#include <vector>

namespace trexhip {

static constexpr float EPS_BN = 1e-5f, EPS_LN = 1e-5f;

// ------------------------------------------------------------------------------------------------
// conv1 forward: [n][80][80][CH] float -> z1 [n][80][80][16] = conv + bias.  Block = 4 rows of one crop, one pixel per thread.
// ------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(320) void k_t_conv1(const float* __restrict__ x, const float* __restrict__ w /*[CH][25][16]*/,
                                                 const float* __restrict__ b, float* __restrict__ z, double* __restrict__ stat_partial /*[block][2][16] or null*/) {
    __shared__ float xs[8 * 84 * CH];
    __shared__ __attribute__((aligned(16))) float ws[CH * 25 * 16];
    const int tid = threadIdx.x, crop = blockIdx.x / 20, row0 = (blockIdx.x % 20) * 4;
    for (int idx = tid; idx < 8 * 84 * CH; idx += 320) {
        const int c = idx % CH, px = (idx / CH) % 84, py = idx / (CH * 84);
        const int iy = row0 + py - 2, ix = px - 2;
        xs[idx] = (iy >= 0 && iy < 80 && ix >= 0 && ix < 80) ? x[(((size_t)crop * 80 + iy) * 80 + ix) * CH + c] : 0.f;
    }
    for (int idx = tid; idx < CH * 25 * 16; idx += 320) ws[idx] = w[idx];
    __syncthreads();
    const int y = tid / 80, xx = tid % 80;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
#pragma unroll 1
    for (int c = 0; c < CH; ++c)
#pragma unroll 1
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const float v = xs[((y + ky) * 84 + xx + kx) * CH + c];
                const float4* wv = reinterpret_cast<const float4*>(ws + (c * 25 + ky * 5 + kx) * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 t = wv[q];
                    acc[4 * q] += v * t.x; acc[4 * q + 1] += v * t.y; acc[4 * q + 2] += v * t.z; acc[4 * q + 3] += v * t.w;
                }
            }
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] += b[k];
    float4* o = reinterpret_cast<float4*>(z + (((size_t)crop * 80 + row0 + y) * 80 + xx) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    if (!stat_partial) return;                                // (uniform)
    // the block's column sums and sums of squares for the BN that follows.  Per wave a reduce-scatter butterfly: at distance 32, 16, 8, 4 a lane
    // keeps half of its channels and hands the other half to its partner, then two plain steps: a lane ends with the sum of channel
    // 8 b5 + 4 b4 + 2 b3 + b2 (b = bits of its number; 17 exchanges per plane instead of 96).  The five waves are added in order through LDS
    __shared__ double sred[5][2][16];
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = pl ? (double)acc[k] * acc[k] : (double)acc[k];
#define T_RS(N, D)                                                                                       \
        {                                                                                                \
            const bool hi = (lane & D) != 0;                                                             \
            _Pragma("unroll") for (int k = 0; k < N; ++k) {                                              \
                const double mine = hi ? v[k + N] : v[k], other = hi ? v[k] : v[k + N];                  \
                v[k] = mine + __shfl_xor(other, D);                                                      \
            }                                                                                            \
        }
        T_RS(8, 32) T_RS(4, 16) T_RS(2, 8) T_RS(1, 4)
#undef T_RS
        v[0] += __shfl_xor(v[0], 2);
        v[0] += __shfl_xor(v[0], 1);
        if ((lane & 3) == 0) sred[wave][pl][((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1)] = v[0];
    }
    __syncthreads();
    if (tid < 32) {
        const int pl = tid >> 4, c = tid & 15;
        double t = 0;
#pragma unroll
        for (int wv = 0; wv < 5; ++wv) t += sred[wv][pl][c];
        stat_partial[((size_t)blockIdx.x * 2 + pl) * 16 + c] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// Reductions over the batch (BN statistics, BN backward sums, bias gradients): every block of the producing kernel leaves its column sums
// as doubles in partial[block][NP][C]; k_t_red_finalize (one workgroup per channel: one L2 round trip, not a chain of them) adds them in
// a fixed order -- same bits every run -- and does what the sum is for.  (Forming the totals in the producing kernel's last block was
// tried: the device-scope fences it needs write back / invalidate the L2 per block and cost 25-110 us per launch.)
// ------------------------------------------------------------------------------------------------
enum { FIN_BN_STATS = 0, FIN_BN_BWD = 1, FIN_BIAS = 2 };
struct FinArgs {
    double count; float momentum;                         // FIN_BN_STATS
    float *o0, *o1, *o2, *o3;                             // FIN_BN_STATS: mean, invstd, run_mean, run_var; FIN_BN_BWD: sums[2][C], d_gamma, d_beta; FIN_BIAS: d_bias
    const int32_t* refused;
};

template <int MODE>
__global__ __launch_bounds__(256) void k_t_red_finalize(const double* __restrict__ partial, const int nblocks, const int C, const FinArgs A) {
    constexpr int NP = MODE == FIN_BIAS ? 1 : 2;
    __shared__ double sh[NP][4];
    const int c = blockIdx.x, tid = threadIdx.x;
    double t[NP];
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) t[pl] = 0;
    for (int b = tid; b < nblocks; b += 256)
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) t[pl] += partial[((size_t)b * NP + pl) * C + c];
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) t[pl] += __shfl_xor(t[pl], d);
        if ((tid & 63) == 0) sh[pl][tid >> 6] = t[pl];
    }
    __syncthreads();
    if (tid) return;
    double tot[NP];
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) tot[pl] = ((sh[pl][0] + sh[pl][1]) + sh[pl][2]) + sh[pl][3];
    if constexpr (MODE == FIN_BN_STATS) {                    // mean, invstd (biased variance, like the normalisation uses); running statistics with the unbiased one
        const double m = tot[0] / A.count;
        double var = tot[1] / A.count - m * m;
        if (var < 0) var = 0;
        A.o0[c] = (float)m;
        A.o1[c] = (float)(1.0 / sqrt(var + (double)EPS_BN));
        const double unbiased = A.count > 1 ? var * A.count / (A.count - 1) : var;
        if (*A.refused) return;                              // a refused step leaves the running statistics alone (k_t_check_targets)
        A.o2[c] = (1.f - A.momentum) * A.o2[c] + A.momentum * (float)m;
        A.o3[c] = (1.f - A.momentum) * A.o3[c] + A.momentum * (float)unbiased;
    } else if constexpr (MODE == FIN_BN_BWD) {               // sums[0][C] = sum dy (= d beta), sums[1][C] = sum dy x-hat (= d gamma)
        const float sd = (float)tot[0], sg = (float)tot[1];
        A.o0[c] = sd; A.o0[C + c] = sg;
        A.o2[c] = sd; A.o1[c] = sg;
    } else {
        A.o0[c] = (float)tot[0];
    }
}

// ------------------------------------------------------------------------------------------------
// batch statistics of z[rows][C]: per-channel sum and sum of squares, double accumulation -> partial[block][2][C] (FIN_BN_STATS)
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void k_t_bn_stats(const float* __restrict__ d, size_t rows, double* __restrict__ partial) {
    constexpr int LC = C / 4, RL = 256 / LC;
    __shared__ double sh[RL * C];
    const int tid = threadIdx.x, cl = tid % LC, rl = tid / LC;
    double a[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (size_t r = (size_t)blockIdx.x * RL + rl; r < rows; r += (size_t)gridDim.x * RL) {
        const float4 v = *reinterpret_cast<const float4*>(d + r * C + cl * 4);
        a[0][0] += v.x; a[0][1] += v.y; a[0][2] += v.z; a[0][3] += v.w;
        a[1][0] += (double)v.x * v.x; a[1][1] += (double)v.y * v.y; a[1][2] += (double)v.z * v.z; a[1][3] += (double)v.w * v.w;
    }
    block_columns<C, 2>(a, sh, partial);
}

// eval mode: normalise with the running statistics
__global__ void k_t_bn_from_running(const float* __restrict__ run_mean, const float* __restrict__ run_var, int C, float* __restrict__ mean, float* __restrict__ invstd) {
    const int c = threadIdx.x;
    if (c >= C) return;
    mean[c] = run_mean[c];
    invstd[c] = (float)(1.0 / sqrt((double)run_var[c] + (double)EPS_BN));
}

// ------------------------------------------------------------------------------------------------
// The head.  (BN + ReLU + pool + dropout with its way back, and fc1 with its two gradients, follow the plane's size: they are train_any.hip's
// k_tany_ kernels at every size, 80x80 included)
// ------------------------------------------------------------------------------------------------
// block reduction of one float over 128 threads, fixed order
__device__ __forceinline__ float block_sum128(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 64; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ float block_max128(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 64; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    return red[0];
}

// one block per sample: fc1 bias + LayerNorm + ReLU + dropout + fc2 + softmax cross entropy, and the way back down to d(fc1 output).
// PLANES = fc1's partial planes in hpart, added here in order: 100 at 80x80 (one per position), 1 at every other size (k_tany_fc1_sum has
// added them)
template <int PLANES>
__global__ __launch_bounds__(128) void k_t_head(const float* __restrict__ hpart, int n, const float* __restrict__ b1, const float* __restrict__ lng,
                                                const float* __restrict__ lnb, const uint8_t* __restrict__ keep /*[n][100]*/, float scale,
                                                const float* __restrict__ w2 /*[C][100]*/, const float* __restrict__ b2, const int32_t* __restrict__ targets,
                                                int classes, float* __restrict__ xhat /*[n][100]*/, float* __restrict__ hd /*[n][100]*/,
                                                float* __restrict__ dl /*[n][C]*/, float* __restrict__ dy /*[n][100]*/, float* __restrict__ dh /*[n][100]*/,
                                                float* __restrict__ loss /*[n]*/, int32_t* __restrict__ correct /*[n]*/, int32_t* __restrict__ bad_target) {
    __shared__ float red[128];
    __shared__ float s_d[100];
    __shared__ float s_dl[1024];
    __shared__ int s_arg[128];
    const int tid = threadIdx.x, s = blockIdx.x;
    const bool act = tid < 100;
    float h = 0.f;
    if (act) {
        h = b1[tid];
        for (int hw = 0; hw < PLANES; ++hw) h += hpart[((size_t)hw * n + s) * 100 + tid];
    }
    const float mean = block_sum128(act ? h : 0.f, red) * 0.01f;
    const float dv = act ? h - mean : 0.f;
    const float var = block_sum128(dv * dv, red) * 0.01f;
    const float rstd = 1.0f / sqrtf(var + EPS_LN);
    float xh = 0.f, y = 0.f, d = 0.f;
    bool kp = false;
    if (act) {
        xh = dv * rstd;
        y = xh * lng[tid] + lnb[tid];
        kp = keep[(size_t)s * 100 + tid] != 0;
        d = kp ? fmaxf(y, 0.f) * scale : 0.f;
        s_d[tid] = d;
        xhat[(size_t)s * 100 + tid] = xh;
        hd[(size_t)s * 100 + tid] = d;
    }
    __syncthreads();
    // logits
    float lmax = -INFINITY;
    int larg = 0x7fffffff;
    for (int c = tid; c < classes; c += 128) {
        float acc = b2[c];
        const float* wr = w2 + (size_t)c * 100;
        for (int j = 0; j < 100; ++j) acc += s_d[j] * wr[j];
        s_dl[c] = acc;
        if (acc > lmax) { lmax = acc; larg = c; }
    }
    const float gmax = block_max128(lmax, red);
    __syncthreads();
    s_arg[tid] = (lmax == gmax) ? larg : 0x7fffffff;       // first index of the maximum, like torch.argmax
    __syncthreads();
    for (int st = 64; st > 0; st >>= 1) {
        if (tid < st) s_arg[tid] = min(s_arg[tid], s_arg[tid + st]);
        __syncthreads();
    }
    int target = targets[s];
    if (target < 0 || target >= classes) target = 0;       // (memory safety only: k_t_check_targets has already refused this step)
    float se = 0.f;
    for (int c = tid; c < classes; c += 128) se += expf(s_dl[c] - gmax);
    const float sum = block_sum128(se, red);
    const float lse = gmax + logf(sum);
    if (tid == 0) {
        loss[s] = lse - s_dl[target];
        correct[s] = s_arg[0] == target ? 1 : 0;
    }
    __syncthreads();
    const float invn = 1.0f / (float)n;
    for (int c = tid; c < classes; c += 128) {
        const float p = expf(s_dl[c] - lse);
        const float gl = (p - (c == target ? 1.f : 0.f)) * invn;
        s_dl[c] = gl;
        dl[(size_t)s * classes + c] = gl;
    }
    __syncthreads();
    float gy = 0.f;
    if (act) {
        float dd = 0.f;
        for (int c = 0; c < classes; ++c) dd += s_dl[c] * w2[(size_t)c * 100 + tid];
        gy = (kp && y > 0.f) ? dd * scale : 0.f;              // through dropout and the ReLU gate: gradient at the LayerNorm output
        dy[(size_t)s * 100 + tid] = gy;
    }
    // LayerNorm backward: dh = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)), dxh = gy * gamma
    const float dxh = act ? gy * lng[tid] : 0.f;
    const float m1 = block_sum128(dxh, red) * 0.01f;
    const float m2 = block_sum128(dxh * xh, red) * 0.01f;
    if (act) dh[(size_t)s * 100 + tid] = rstd * (dxh - m1 - xh * m2);
}

// the head of a prediction (trexhip_train_predict_device): k_t_head's forward half with nothing dropped -- fc1 bias + LayerNorm + ReLU + fc2, the
// same expressions in the same order -- and the softmax row expf(l - lse), as k_t_head forms p.  No targets, none of the backward buffers
template <int PLANES>
__global__ __launch_bounds__(128) void k_t_head_eval(const float* __restrict__ hpart, int n, const float* __restrict__ b1, const float* __restrict__ lng,
                                                     const float* __restrict__ lnb, const float* __restrict__ w2 /*[C][100]*/, const float* __restrict__ b2,
                                                     int classes, float* __restrict__ probs /*[n][C]*/) {
    __shared__ float red[128];
    __shared__ float s_d[100];
    __shared__ float s_dl[1024];
    const int tid = threadIdx.x, s = blockIdx.x;
    const bool act = tid < 100;
    float h = 0.f;
    if (act) {
        h = b1[tid];
        for (int hw = 0; hw < PLANES; ++hw) h += hpart[((size_t)hw * n + s) * 100 + tid];
    }
    const float mean = block_sum128(act ? h : 0.f, red) * 0.01f;
    const float dv = act ? h - mean : 0.f;
    const float var = block_sum128(dv * dv, red) * 0.01f;
    const float rstd = 1.0f / sqrtf(var + EPS_LN);
    if (act) {
        const float xh = dv * rstd;
        const float y = xh * lng[tid] + lnb[tid];
        s_d[tid] = fmaxf(y, 0.f);
    }
    __syncthreads();
    float lmax = -INFINITY;
    for (int c = tid; c < classes; c += 128) {
        float acc = b2[c];
        const float* wr = w2 + (size_t)c * 100;
        for (int j = 0; j < 100; ++j) acc += s_d[j] * wr[j];
        s_dl[c] = acc;
        if (acc > lmax) lmax = acc;
    }
    const float gmax = block_max128(lmax, red);
    float se = 0.f;
    for (int c = tid; c < classes; c += 128) se += expf(s_dl[c] - gmax);
    const float sum = block_sum128(se, red);
    const float lse = gmax + logf(sum);
    for (int c = tid; c < classes; c += 128) probs[(size_t)s * classes + c] = expf(s_dl[c] - lse);
}

// parameter gradients of the head: fc2 weight / bias, LayerNorm gamma / beta, fc1 bias; one thread per element, samples in order
__global__ __launch_bounds__(256) void k_t_head_grads(const float* __restrict__ dl, const float* __restrict__ hd, const float* __restrict__ dy,
                                                      const float* __restrict__ xhat, const float* __restrict__ dh, int n, int classes,
                                                      float* __restrict__ g_w2, float* __restrict__ g_b2, float* __restrict__ g_lng, float* __restrict__ g_lnb,
                                                      float* __restrict__ g_b1) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nw = classes * 100;
    // sums over the samples in order, eight samples' operands in flight (one dependent L2 round trip per sample otherwise)
#define HG_SUM(expr_a_, expr_b_)                                                                                                 \
    for (int s0 = 0; s0 < n; s0 += 8) {                                                                                          \
        float va_[8], vb_[8];                                                                                                    \
        _Pragma("unroll") for (int k = 0; k < 8; ++k) { const int s = s0 + k < n ? s0 + k : n - 1; va_[k] = (expr_a_); vb_[k] = (expr_b_); } \
        _Pragma("unroll") for (int k = 0; k < 8; ++k) if (s0 + k < n) acc += va_[k] * vb_[k];                                     \
    }
    if (idx < nw) {
        const int c = idx / 100, j = idx % 100;
        float acc = 0.f;
        HG_SUM(dl[(size_t)s * classes + c], hd[(size_t)s * 100 + j])
        g_w2[idx] = acc;
    } else if (idx < nw + classes) {
        const int c = idx - nw;
        float acc = 0.f;
        HG_SUM(dl[(size_t)s * classes + c], 1.f)
        g_b2[c] = acc;
    } else if (idx < nw + classes + 300) {
        const int k3 = idx - nw - classes, j = k3 % 100, which = k3 / 100;
        float acc = 0.f;
        if (which == 0) { HG_SUM(dy[(size_t)s * 100 + j], xhat[(size_t)s * 100 + j]) g_lng[j] = acc; }
        else if (which == 1) { HG_SUM(dy[(size_t)s * 100 + j], 1.f) g_lnb[j] = acc; }
        else { HG_SUM(dh[(size_t)s * 100 + j], 1.f) g_b1[j] = acc; }
    }
#undef HG_SUM
}

// ------------------------------------------------------------------------------------------------
// conv2 / conv3 forward and data gradients on the 16-bit matrix cores (precision 0, the default): the inference path's arithmetic --
// x = h1 + h2 with two fp16 pieces (22 mantissa bits), products h2 g1, h1 g2, h1 g1 on v_mfma_f32_32x32x16_f16, fp32 accumulation --
// at a fifth of the fp32-MFMA time (k_conv5<RAW>, precision 1).  fp16 cannot hold every fp32 value, so both operands carry a power-of-two
// scale: the inputs one per workgroup and 16 / 32-channel chunk, from the largest |value| of the patch it stages (largest scaled input in
// [2^13, 2^14)); the weights one per layer, from the pack kernel (largest scaled weight in [2^7, 2^8)).  Nothing overflows, and what
// underflows is below 2^-27 of the patch's / the layer's largest entry.  25 shifted GEMMs: patch in LDS, weight fragments L2 -> VGPR, no barrier inside a chunk.
// ------------------------------------------------------------------------------------------------
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float pow2_scale_for(const uint32_t maxbits, const int target_exp) {   // 2^k with max * 2^k in [2^target, 2^(target + 1))
    if (maxbits == 0u) return 1.f;
    int e = (int)((maxbits >> 23) & 0xffu) - 127;
    int k = target_exp - e;
    k = k < -100 ? -100 : (k > 100 ? 100 : k);
    return __uint_as_float((uint32_t)(127 + k) << 23);
}
__device__ __forceinline__ void split2h_t(const float x, uint32_t& h1, uint32_t& h2) {
    const _Float16 a = (_Float16)x;
    const _Float16 b = (_Float16)(x - (float)a);
    h1 = (uint32_t)__builtin_bit_cast(uint16_t, a); h2 = (uint32_t)__builtin_bit_cast(uint16_t, b);
}

template <int CI, int CO, int S, int ROWS, int CIC>
struct ConvGeomH {
    static constexpr int PW = S + 4, PH = ROWS + 4;
    static constexpr int PSTRIDE = CIC * 2 + 16;                      // bytes per pixel (data + 16 pad: odd multiple of 16)
    static constexpr int PATCH = PH * PW * PSTRIDE;                   // bytes per piece
    static constexpr int BT = 2 * (CIC / 8) * CO * 16;                // bytes per weight tile: 2 pieces x CIC / 8 k-octets x CO x 16 B
    static constexpr int NPIX = ROWS * S;
    static constexpr int MT = (NPIX + 31) / 32, NT = CO / 32, WM = 8 / NT, TPW = (MT + WM - 1) / WM;
    static constexpr int LDS_BYTES = 2 * PATCH;
    static constexpr int BPC = S / ROWS;
    static_assert(CO % 32 == 0 && 8 % NT == 0 && CIC % 16 == 0 && CI % CIC == 0 && LDS_BYTES <= 160 * 1024, "shapes");
};

template <int CI, int CO, int S, int ROWS, int CIC, int COUT>
__global__ __launch_bounds__(512) void k_t_conv5_h2(const float* __restrict__ in /*[N][S][S][CI]*/, const uint4* __restrict__ wp /*[CI/CIC][25][2][CIC/8][CO] x 16 B*/,
                                                    const float* __restrict__ bias /*[COUT] or null*/, float* __restrict__ out /*[N][S][S][COUT]*/,
                                                    const float* __restrict__ w_scale, double* __restrict__ stat_partial /*[block][2][CO] or null*/) {
    using G = ConvGeomH<CI, CO, S, ROWS, CIC>;
    constexpr int Q4 = CIC / 4, KO = CIC / 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t hlds[];
    uint8_t* patch = hlds;                       // 2 pieces
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = wave % G::NT, mg = wave / G::NT;
    const int crop = blockIdx.x / G::BPC, row0 = (blockIdx.x % G::BPC) * ROWS;
    __shared__ float s_red[8];
    float in_scale = 1.f;                                             // of the chunk staged last
    int aoff[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        int p = (mg + G::WM * m) * 32 + j;                             // row-major pixel of the band
        p = p < G::NPIX ? p : G::NPIX - 1;
        aoff[m] = ((p / S) * G::PW + p % S) * G::PSTRIDE + h * 16;
    }
    f32x16 acc[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    const float* inc = in + (size_t)crop * S * S * CI;
    constexpr int NITEM = G::PH * G::PW * Q4, NLD = (NITEM + 511) / 512;  // Q4 float4 per pixel; float4 per thread and chunk
    constexpr int KS = CIC / 16, BV = G::BT / 16;
    const uint4* wl = wp + (h * CO + n * 32 + j);                      // this lane's fragments: + tap * BV + 2 ks CO (+ KO CO: second piece)
    for (int cc = 0; cc < CI / CIC; ++cc) {
        const uint4* wsrc = wl + (size_t)cc * 25 * BV;
        uint4 bq[3][KS][2];
        auto fetch = [&](uint4 (&d)[KS][2], const int tap) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) { d[ks][0] = wsrc[tap * BV + 2 * ks * CO]; d[ks][1] = wsrc[tap * BV + 2 * ks * CO + KO * CO]; }
        };
        fetch(bq[0], 0);
        fetch(bq[1], 1);
        __syncthreads();
        // the chunk's patch: loaded into registers, its largest |value| found (wave shuffle + 8 LDS words), scaled by the power of two that
        // puts that value into [2^13, 2^14), split and stored.  A chunk with another scale than the one before rescales the accumulators
        // (a power of two: exact)
        float4 v[NLD];
        float lm = 0.f;
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int idx = tid + u * 512;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < NITEM) {
                const int q = idx % Q4, px = idx / Q4;
                const int py = px / G::PW, pxx = px - py * G::PW;
                const int iy = row0 + py - 2, ix = pxx - 2;
                if (iy >= 0 && iy < S && ix >= 0 && ix < S) v[u] = *reinterpret_cast<const float4*>(inc + ((size_t)iy * S + ix) * CI + cc * CIC + q * 4);
                lm = fmaxf(lm, fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) lm = fmaxf(lm, __shfl_xor(lm, d));
        if (lane == 0) s_red[wave] = lm;
        __syncthreads();
        float bm = s_red[0];
#pragma unroll
        for (int w = 1; w < 8; ++w) bm = fmaxf(bm, s_red[w]);
        const float sc = pow2_scale_for(__float_as_uint(bm), 13);
        if (cc > 0 && sc != in_scale) {
            const float f = sc / in_scale;
#pragma unroll
            for (int m = 0; m < G::TPW; ++m) acc[m] *= f;
        }
        in_scale = sc;
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int idx = tid + u * 512;
            if (idx < NITEM) {
                const int q = idx % Q4, px = idx / Q4;
                uint32_t a1[4], a2[4];
                split2h_t(v[u].x * sc, a1[0], a2[0]); split2h_t(v[u].y * sc, a1[1], a2[1]);
                split2h_t(v[u].z * sc, a1[2], a2[2]); split2h_t(v[u].w * sc, a1[3], a2[3]);
                uint8_t* d = patch + px * G::PSTRIDE + q * 8;
                *reinterpret_cast<uint2*>(d) = make_uint2(a1[0] | (a1[1] << 16), a1[2] | (a1[3] << 16));
                *reinterpret_cast<uint2*>(d + G::PATCH) = make_uint2(a2[0] | (a2[1] << 16), a2[2] | (a2[3] << 16));
            }
        }
        __syncthreads();
        // the tap loop runs without barriers: the patch is read-only until the next chunk, and each wave takes its weight fragments L2 -> VGPR
        // straight from the packed image, two taps ahead (through LDS they cost a barrier per tap: 1.4 us per tap against 0.7 of MFMAs)
#pragma unroll
        for (int tap = 0; tap < 25; ++tap) {
            if (tap + 2 < 25) fetch(bq[(tap + 2) % 3], tap + 2);
            const uint8_t* asrc = patch + ((tap / 5) * G::PW + (tap % 5)) * G::PSTRIDE;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {                              // one 16-deep MFMA step per 16 input channels
                const h16x8 b1 = __builtin_bit_cast(h16x8, bq[tap % 3][ks][0]);
                const h16x8 b2 = __builtin_bit_cast(h16x8, bq[tap % 3][ks][1]);
#pragma unroll
                for (int m = 0; m < G::TPW; ++m) {
                    const h16x8 p1 = __builtin_bit_cast(h16x8, *reinterpret_cast<const uint4*>(asrc + aoff[m] + ks * 32));
                    const h16x8 p2 = __builtin_bit_cast(h16x8, *reinterpret_cast<const uint4*>(asrc + aoff[m] + ks * 32 + G::PATCH));
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p2, b1, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p1, b2, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p1, b1, acc[m], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();                                                      // (the epilogue's statistics reuse the patch)
    const int co = n * 32 + j;
    if (co >= COUT && !(COUT == CO && stat_partial)) return;
    const float out_scale = 1.0f / (in_scale * *w_scale);             // powers of two: exact
    const float bz = bias ? bias[co] : 0.f;
    float* oc = out + ((size_t)crop * S * S + (size_t)row0 * S) * COUT;
    double sv = 0, sq = 0;                                            // this lane's share of the channel's sum and sum of squares (the BN that follows)
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int mt = mg + G::WM * m;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = mt * 32 + 8 * (r / 4) + 4 * h + (r % 4);        // accumulator r of lane (j, h) is row 8 (r / 4) + 4 h + r % 4
            if (p < G::NPIX) {
                const float v = acc[m][r] * out_scale + bz;
                oc[(size_t)p * COUT + co] = v;
                if (COUT == CO) { sv += v; sq += (double)v * v; }
            }
        }
    }
    if constexpr (COUT == CO) {
        if (!stat_partial) return;                                    // (uniform)
        // the 2 WM lanes of a channel through LDS (the patch is dead: the tap loop ended on a barrier), added in a fixed order
        double* sh = reinterpret_cast<double*>(hlds);
        const int slot = mg * 2 + h;
        sh[slot * CO + co] = sv;
        sh[(2 * G::WM + slot) * CO + co] = sq;
        __syncthreads();
        if (tid < 2 * CO) {
            const int pl = tid / CO, c = tid % CO;
            double t = 0;
#pragma unroll
            for (int k = 0; k < 2 * G::WM; ++k) t += sh[(pl * 2 * G::WM + k) * CO + c];
            stat_partial[((size_t)blockIdx.x * 2 + pl) * CO + c] = t;
        }
    }
}

// weights of one layer -> the B-operand image of k_t_conv5_h2, both directions in one launch: [dir][k / CICK][tap][piece][(k % CICK) / 8][n] x 16 B
// (8 consecutive k per 16 bytes).  dir 0 = forward: k = ci, n = co, w(ci, tap, co); dir 1 = data gradient: k = co, n = ci (padded to NP1
// columns), w(ci, 24 - tap, co).  Parameter layout of w: [ci / CICP][tap][ci % CICP][co].  Every block finds the tensor's largest |w| itself
// (the same value in every block), block 0 writes the scale.
__global__ __launch_bounds__(1024) void k_t_pack_h2(const float* __restrict__ w, const int CI, const int CO, const int CICP, const int CICK0, const int CICK1,
                                                    const int NP1, uint4* __restrict__ out0, uint4* __restrict__ out1, float* __restrict__ w_scale) {
    __shared__ float red[1024];
    const int total4 = 25 * CI * CO / 4;
    float m = 0.f;
#pragma unroll 4
    for (int i = threadIdx.x; i < total4; i += 1024) {
        const float4 v = reinterpret_cast<const float4*>(w)[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int d = 512; d >= 1; d >>= 1) { if ((int)threadIdx.x < d) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + d]); __syncthreads(); }
    const float sc = pow2_scale_for(__float_as_uint(red[0]), 7);
    if (blockIdx.x == 0 && threadIdx.x == 0) *w_scale = sc;
    auto wat = [&](int ci, int tap, int co) -> float { return w[(((size_t)(ci / CICP) * 25 + tap) * CICP + ci % CICP) * CO + co]; };
    const int n0 = (CI / 8) * 25 * CO, n1 = (CO / 8) * 25 * NP1;         // 16-byte units per piece
    for (int u = blockIdx.x * 1024 + threadIdx.x; u < n0 + n1; u += gridDim.x * 1024) {
        const bool d1 = u >= n0;
        const int v = d1 ? u - n0 : u;
        const int K = d1 ? CO : CI, N = d1 ? NP1 : CO, CK = d1 ? CICK1 : CICK0;
        const int nn = v % N, ko = (v / N) % (CK / 8), tap = (v / (N * (CK / 8))) % 25, cc = v / (N * (CK / 8) * 25);
        (void)K;
        uint32_t h1[8], h2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = cc * CK + ko * 8 + e;
            float x = 0.f;
            if (!d1) x = wat(k, tap, nn);
            else if (nn < CI) x = wat(nn, 24 - tap, k);
            split2h_t(x * sc, h1[e], h2[e]);
        }
        uint4* o = (d1 ? out1 : out0) + ((size_t)(cc * 25 + tap) * 2 * (CK / 8) + ko) * N + nn;
        o[0] = make_uint4(h1[0] | (h1[1] << 16), h1[2] | (h1[3] << 16), h1[4] | (h1[5] << 16), h1[6] | (h1[7] << 16));
        o[(size_t)(CK / 8) * N] = make_uint4(h2[0] | (h2[1] << 16), h2[2] | (h2[3] << 16), h2[4] | (h2[5] << 16), h2[6] | (h2[7] << 16));
    }
}

// ------------------------------------------------------------------------------------------------
// convolution weight gradient on fp32 MFMA: dW[tap][ci][co] = sum over (crop, y, x) a[crop][y+ky-2][x+kx-2][ci] * dz[crop][y][x][co].
// One 32x32x2 MFMA step contracts over two neighbouring pixels: A = activations at the taps' shifts, B = dz.
//   * block = one kernel row ky x one slice of CIS input channels x one slice of COS output channels x one share of the work units
//     (unit = ROWS output rows of one crop).  It stages the unit's dz slice [ROWS * S pixels][COS] and the ROWS activation rows the kernel
//     row needs ([ROWS][S][CIS], rows outside the crop skipped) in LDS with 16-byte loads -- round 2 fetched every MFMA operand as a
//     4-byte load straight from L2 and ran at half its MFMA count -- and all 8 waves read their operands from there;
//   * M space of a kernel row = [5 kx][CIS] rows in MT tiles of 32 (conv3: CIS = 32, tile = kx; conv2: CIS = 16, 80 rows in 3 tiles);
//     a wave holds MT x (COS / 32) accumulator tiles and takes every 8th pixel pair; one dz fragment serves the MT shifted A fragments;
//   * the waves' sums are added in wave order through LDS: part[share][tap][ci][co], summed over the shares by k_t_wgrad_reduce --
//     the same bits every run.
// ------------------------------------------------------------------------------------------------
template <int CI, int CO, int S, int CIS, int COS, int MT, int ROWS>
struct WgradGeom {
    static constexpr int NT = COS / 32, NB = S / ROWS, WAVES = 8;
    static constexpr int NCS = CI / CIS, NOS = CO / COS, TYPES = 5 * NCS * NOS;
    static constexpr int DZ_FLOATS = ROWS * S * COS, A_FLOATS = ROWS * S * CIS, UNIT_FLOATS = DZ_FLOATS + A_FLOATS;
    static constexpr int SUM_FLOATS = MT * NT * 16 * 64;
    static constexpr int LDS_BYTES = (2 * UNIT_FLOATS > SUM_FLOATS ? 2 * UNIT_FLOATS : SUM_FLOATS) * 4;
    static_assert(S % ROWS == 0 && S % 2 == 0 && CI % CIS == 0 && CO % COS == 0 && COS % 32 == 0 && MT * 32 >= 5 * CIS, "shapes");
    static_assert(LDS_BYTES <= 160 * 1024 && (DZ_FLOATS * 4) % 1024 == 0 && 1024 % (COS * 4) == 0 && 1024 % (CIS * 4) == 0, "LDS");
};

// one LDS-DMA instruction: 64 lanes x 16 bytes from the lanes' global addresses to LDS [lds_addr, lds_addr + 1024).  Raw, so that the compiler's
// wait-count pass does not know of it: it cannot tell the two LDS buffers apart and would drain the DMA in front of every LDS read.
__device__ __forceinline__ void dma16_raw(const void* gptr, const uint32_t lds_addr) {
    uint32_t keep;                                                         // M0 is the compiler's: handed back as found
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_addr), "v"(gptr) : "memory");
}

template <int CI, int CO, int S, int CIS, int COS, int MT, int ROWS>
__global__ __launch_bounds__(512) void k_t_wgrad(const float* __restrict__ a /*[n][S][S][CI]*/, const float* __restrict__ dz /*[n][S][S][CO]*/,
                                                 float* __restrict__ part, int n) {
    using G = WgradGeom<CI, CO, S, CIS, COS, MT, ROWS>;
    constexpr int NT = G::NT, NB = G::NB, WAVES = G::WAVES;
    extern __shared__ __attribute__((aligned(16))) float wg_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 31, h = lane >> 5;
    const int type = blockIdx.x, ky = type / (G::NCS * G::NOS), cs = (type / G::NOS) % G::NCS, os = type % G::NOS;
    const int share = blockIdx.y, shares = gridDim.y, units = n * NB;
    int kx[MT], cc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int mi = mt * 32 + j;
        kx[mt] = mi / CIS; cc[mt] = mi % CIS;                              // rows past the 5th tap stay zero
    }
    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    // a unit travels L2 -> the other LDS buffer by LDS-DMA while the MFMAs of the previous unit run: 1-KB pieces (4 dz pixels, or
    // 1024 / (4 CIS) activation pixels), dealt out to the 8 waves.  Activation rows outside the crop are fetched from a clamped row
    // and never read.
    const uint32_t lds0 = (uint32_t)(uintptr_t)wg_lds;
#define WG_FETCH(u_, buf_)                                                                                                       \
    do {                                                                                                                         \
        const int crop_ = (u_) / NB, y0_ = ((u_) % NB) * ROWS;                                                                   \
        const uint8_t* src_ = reinterpret_cast<const uint8_t*>(dz + ((size_t)crop_ * S * S + (size_t)y0_ * S) * CO + os * COS);  \
        const uint32_t dst_ = lds0 + (buf_) * G::UNIT_FLOATS * 4;                                                                \
        _Pragma("unroll 1") for (int k_ = wave; k_ < G::DZ_FLOATS * 4 / 1024; k_ += WAVES)                                        \
            dma16_raw(src_ + (size_t)(k_ * (1024 / (COS * 4)) + lane / (COS / 4)) * (CO * 4) + (lane % (COS / 4)) * 16, dst_ + k_ * 1024); \
        const uint8_t* asrc_ = reinterpret_cast<const uint8_t*>(a + (size_t)crop_ * S * S * CI + cs * CIS);                       \
        constexpr int PPI_ = 1024 / (CIS * 4);                           /* pixels per piece */                                  \
        _Pragma("unroll 1") for (int k_ = wave; k_ < (G::A_FLOATS * 4 + 1023) / 1024; k_ += WAVES) {                              \
            const int px_ = k_ * PPI_ + lane / (CIS / 4);                                                                        \
            if (px_ < ROWS * S) {                                                                                                \
                int ys_ = y0_ + px_ / S + ky - 2;                                                                                \
                ys_ = ys_ < 0 ? 0 : (ys_ >= S ? S - 1 : ys_);                                                                    \
                dma16_raw(asrc_ + ((size_t)ys_ * S + px_ % S) * (CI * 4) + (lane % (CIS / 4)) * 16, dst_ + G::DZ_FLOATS * 4 + k_ * 1024); \
            }                                                                                                                    \
        }                                                                                                                        \
    } while (0)
    int u = share;
    if (u < units) WG_FETCH(u, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (; u < units; u += shares) {
        const int un = u + shares;
        if (un < units) WG_FETCH(un, cur ^ 1);                             // that buffer's readers finished before the previous barrier
        const float* dzl = wg_lds + cur * G::UNIT_FLOATS;
        const float* al = dzl + G::DZ_FLOATS;
        // rows of the unit whose activation row y + ky - 2 lies inside the crop (the others add nothing)
        const int y0 = (u % NB) * ROWS;
        int r_lo = 2 - ky - y0, r_hi = S + 2 - ky - y0;
        r_lo = r_lo < 0 ? 0 : r_lo; r_hi = r_hi > ROWS ? ROWS : r_hi;
        const int nq = (r_hi - r_lo) * (S / 2);
        // operands of pixel pair q: the dz fragments and the MT shifted activation fragments (both pixels of a pair lie in one row: S is even)
#define WG_OPS(q_, av_, bv_)                                                                                                     \
        do {                                                                                                                     \
            const int r_ = r_lo + (q_) / (S / 2), x_ = 2 * ((q_) % (S / 2)) + h;                                                 \
            _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) bv_[nt] = dzl[(r_ * S + x_) * COS + nt * 32 + j];                   \
            _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) {                                                                  \
                const int xs_ = x_ + kx[mt] - 2;                                                                                 \
                const float v_ = al[(r_ * S + (xs_ < 0 ? 0 : (xs_ >= S ? S - 1 : xs_))) * CIS + cc[mt]];                          \
                av_[mt] = (kx[mt] < 5 && xs_ >= 0 && xs_ < S) ? v_ : 0.f;                                                        \
            }                                                                                                                    \
        } while (0)
        float av[MT], bv[NT];
        if (wave < nq) WG_OPS(wave, av, bv);
        for (int q = wave; q < nq; q += WAVES) {
            float avn[MT], bvn[NT];
            const int qn = q + WAVES < nq ? q + WAVES : q;                 // the next pair's operands are read under this pair's MFMAs
            WG_OPS(qn, avn, bvn);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = avn[mt];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = bvn[nt];
        }
#undef WG_OPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // this wave's pieces of the next unit have landed ...
        __syncthreads();                                                   // ... everyone's, and everyone is done with this unit
        cur ^= 1;
    }
#undef WG_FETCH
    // the waves' sums are added in wave order through LDS: one partial per block, the same bits every run
    __syncthreads();
    float* sum = wg_lds;
    for (int w = 0; w < WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float* d = sum + ((mt * NT + nt) * 16 + r) * 64 + lane;
                        *d = w == 0 ? acc[mt][nt][r] : *d + acc[mt][nt][r];
                    }
        }
        __syncthreads();
    }
    float* pp = part + (size_t)share * 25 * CI * CO;
    for (int e = tid; e < G::SUM_FLOATS; e += WAVES * 64) {
        const int ln = e & 63, r = (e >> 6) & 15, t = e >> 10, nt = t % NT, mt = t / NT;
        const int mi = mt * 32 + 8 * (r / 4) + 4 * (ln >> 5) + (r % 4);     // accumulator r of lane (j, h) is row 8 (r / 4) + 4 h + r % 4
        const int k = mi / CIS, c = cs * CIS + mi % CIS;
        if (k < 5) pp[((size_t)(ky * 5 + k) * CI + c) * CO + os * COS + nt * 32 + (ln & 31)] = sum[e];
    }
}

// ------------------------------------------------------------------------------------------------
// the same weight gradients in the fp16 two-piece split arithmetic (precision 0): v_mfma_f32_32x32x16_f16 contracts SIXTEEN pixels per step
// (three products per term), a fifth of the fp32-MFMA time -- the kernel is then bound by staging, so a workgroup stages a unit once for
// ALL 25 taps:
//   * block = a slice of CIS input channels x a slice of 64 output channels x a share of the units (unit = ROWS output rows of a crop);
//     10 waves = 5 kernel rows x 2 output-channel tiles, a wave holds the 5 kx tiles (conv2: 80 rows = 5 kx x 16 channels in 3 tiles) of
//     its kernel row and walks over ALL pixel segments of the unit: no sum across waves;
//   * operands: a [ROWS + 4 rows][x + 2 .. halo][CIS] and dz [ROWS][x (padded to 8)][64] as two fp16 planes each, [pixel][channel] as they lie
//     in memory; the MFMA wants 8 consecutive PIXELS per lane for one channel -- ds_read_b64_tr_b16 delivers exactly that transpose (a
//     16-lane group reads 4 pixels x 16 channels; lane l supplies pixel l / 4, channels 4 (l % 4) .. and receives channel l of the 4 pixels);
//     a K step = two 8-pixel segments (lanes 0..31 / 32..63), shifted by kx - 2 along x for the A operand (zero halo columns), rows
//     outside the crop are zero rows;
//   * fp16 range: a unit's activations and gradients are scaled by powers of two from their largest |value| (kept while that stays inside
//     [2^10, 2^15)); a change rescales the accumulators (exact).
// ------------------------------------------------------------------------------------------------
typedef __fp16 fh4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ h16x8 tr_frag(const uint8_t* p, const int second_off) {
    struct { fh4 lo, hi; } v;
    v.lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fh4*)(p));
    v.hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fh4*)(p + second_off));
    return __builtin_bit_cast(h16x8, v);
}

template <int CI, int CO, int S, int CIS, int ROWS>
struct WgradHGeom {
    static constexpr int COS = 64, NT = 2, MT = (5 * CIS + 31) / 32, WAVES = 10, NTHR = WAVES * 64;
    static constexpr int SEGS = (S + 7) / 8, DW = SEGS * 8, PW = DW + 4, AR = ROWS + 4;
    static constexpr int A_BYTES = AR * PW * CIS * 2, DZ_BYTES = ROWS * DW * COS * 2;          // per piece
    static constexpr int LDS_BYTES = 2 * A_BYTES + 2 * DZ_BYTES;
    static constexpr int NSEG = ROWS * SEGS;
    static constexpr int NCS = CI / CIS, NOS = CO / COS, TYPES = NCS * NOS, NB = S / ROWS;
    static constexpr int NA4 = AR * S * CIS / 4, ND4 = ROWS * S * COS / 4, NLA = (NA4 + NTHR - 1) / NTHR, NLD = (ND4 + NTHR - 1) / NTHR;
    static_assert(NSEG % 2 == 0 && S % ROWS == 0 && CI % CIS == 0 && CO % COS == 0 && CIS % 16 == 0 && LDS_BYTES % 16 == 0 && LDS_BYTES <= 160 * 1024, "shapes");
};

template <int CI, int CO, int S, int CIS, int ROWS>
__global__ __launch_bounds__(640) void k_t_wgrad_h2(const float* __restrict__ a /*[n][S][S][CI]*/, const float* __restrict__ dz /*[n][S][S][CO]*/,
                                                    float* __restrict__ part, int n) {
    using G = WgradHGeom<CI, CO, S, CIS, ROWS>;
    constexpr int COS = G::COS, MT = G::MT, PW = G::PW, DW = G::DW, SEGS = G::SEGS;
    extern __shared__ __attribute__((aligned(16))) uint8_t wh_lds[];
    __shared__ float s_red[G::WAVES][2];
    uint8_t* const ap = wh_lds;                                          // two pieces, A_BYTES apart
    uint8_t* const dp = wh_lds + 2 * G::A_BYTES;                         // two pieces, DZ_BYTES apart
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5, g16 = (lane >> 4) & 1, l16 = lane & 15;
    const int ky = wave % 5, ntw = wave / 5;
    const int cs = blockIdx.x / G::NOS, os = blockIdx.x % G::NOS;
    const int share = blockIdx.y, shares = gridDim.y, units = n * G::NB;
    for (int i = tid; i < G::LDS_BYTES / 16; i += G::NTHR) reinterpret_cast<uint4*>(wh_lds)[i] = make_uint4(0, 0, 0, 0);   // halo and pad columns stay zero
    // lane constants of the transposing reads: tile i = rows i * 32 + 16 g16 + (l16): kernel column kx = row / CIS, channel = row % CIS
    int a_lane[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m0 = i * 32 + 16 * g16;
        int kx = m0 / CIS;
        kx = kx < 5 ? kx : 4;                                            // rows past the fifth tap are never written out
        a_lane[i] = (((l16 >> 2) + kx) * CIS + m0 % CIS + 4 * (l16 & 3)) * 2;
    }
    const int d_lane = ((l16 >> 2) * COS + ntw * 32 + 16 * g16 + 4 * (l16 & 3)) * 2;
    f32x16 acc[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float sa = 1.f, sd = 1.f;                                            // scales of the unit staged last
    for (int u = share; u < units; u += shares) {
        const int crop = u / G::NB, y0 = (u % G::NB) * ROWS;
        const float* asrc = a + (size_t)crop * S * S * CI + cs * CIS;
        const float* dsrc = dz + ((size_t)crop * S * S + (size_t)y0 * S) * CO + os * COS;
        float4 va[G::NLA], vd[G::NLD];
        float ma = 0.f, md = 0.f;
#pragma unroll
        for (int k = 0; k < G::NLA; ++k) {
            const int idx = tid + k * G::NTHR;
            va[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < G::NA4) {
                const int c4 = idx % (CIS / 4), x = (idx / (CIS / 4)) % S, ar = idx / (CIS / 4 * S);
                const int y = y0 - 2 + ar;
                if (y >= 0 && y < S) va[k] = *reinterpret_cast<const float4*>(asrc + ((size_t)y * S + x) * CI + c4 * 4);
                ma = fmaxf(ma, fmaxf(fmaxf(fabsf(va[k].x), fabsf(va[k].y)), fmaxf(fabsf(va[k].z), fabsf(va[k].w))));
            }
        }
#pragma unroll
        for (int k = 0; k < G::NLD; ++k) {
            const int idx = tid + k * G::NTHR;
            vd[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < G::ND4) {
                const int c4 = idx % (COS / 4), px = idx / (COS / 4);
                vd[k] = *reinterpret_cast<const float4*>(dsrc + (size_t)px * CO + c4 * 4);
                md = fmaxf(md, fmaxf(fmaxf(fabsf(vd[k].x), fabsf(vd[k].y)), fmaxf(fabsf(vd[k].z), fabsf(vd[k].w))));
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { ma = fmaxf(ma, __shfl_xor(ma, d)); md = fmaxf(md, __shfl_xor(md, d)); }
        __syncthreads();                                                 // the previous unit's readers are done (and s_red is free)
        if (lane == 0) { s_red[wave][0] = ma; s_red[wave][1] = md; }
        __syncthreads();
        ma = s_red[0][0]; md = s_red[0][1];
#pragma unroll
        for (int w = 1; w < G::WAVES; ++w) { ma = fmaxf(ma, s_red[w][0]); md = fmaxf(md, s_red[w][1]); }
        // keep a scale while the unit's largest value stays inside [2^10, 2^15) with it: few rescalings of the accumulators
        float na = sa, nd = sd;
        if (!(ma * sa >= 1024.f && ma * sa < 32768.f) && ma > 0.f) na = pow2_scale_for(__float_as_uint(ma), 13);
        if (!(md * sd >= 1024.f && md * sd < 32768.f) && md > 0.f) nd = pow2_scale_for(__float_as_uint(md), 13);
        if (na != sa || nd != sd) {
            const float f = (na / sa) * (nd / sd);
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i] *= f;
            sa = na; sd = nd;
        }
#pragma unroll
        for (int k = 0; k < G::NLA; ++k) {
            const int idx = tid + k * G::NTHR;
            if (idx < G::NA4) {
                const int c4 = idx % (CIS / 4), x = (idx / (CIS / 4)) % S, ar = idx / (CIS / 4 * S);
                uint32_t p1[4], p2[4];
                split2h_t(va[k].x * sa, p1[0], p2[0]); split2h_t(va[k].y * sa, p1[1], p2[1]);
                split2h_t(va[k].z * sa, p1[2], p2[2]); split2h_t(va[k].w * sa, p1[3], p2[3]);
                uint8_t* d = ap + ((ar * PW + x + 2) * CIS + c4 * 4) * 2;
                *reinterpret_cast<uint2*>(d) = make_uint2(p1[0] | (p1[1] << 16), p1[2] | (p1[3] << 16));
                *reinterpret_cast<uint2*>(d + G::A_BYTES) = make_uint2(p2[0] | (p2[1] << 16), p2[2] | (p2[3] << 16));
            }
        }
#pragma unroll
        for (int k = 0; k < G::NLD; ++k) {
            const int idx = tid + k * G::NTHR;
            if (idx < G::ND4) {
                const int c4 = idx % (COS / 4), px = idx / (COS / 4), x = px % S, r = px / S;
                uint32_t p1[4], p2[4];
                split2h_t(vd[k].x * sd, p1[0], p2[0]); split2h_t(vd[k].y * sd, p1[1], p2[1]);
                split2h_t(vd[k].z * sd, p1[2], p2[2]); split2h_t(vd[k].w * sd, p1[3], p2[3]);
                uint8_t* d = dp + ((r * DW + x) * COS + c4 * 4) * 2;
                *reinterpret_cast<uint2*>(d) = make_uint2(p1[0] | (p1[1] << 16), p1[2] | (p1[3] << 16));
                *reinterpret_cast<uint2*>(d + G::DZ_BYTES) = make_uint2(p2[0] | (p2[1] << 16), p2[2] | (p2[3] << 16));
            }
        }
        __syncthreads();
        for (int p = 0; p < G::NSEG / 2; ++p) {
            const int sg = 2 * p + h, r = sg / SEGS, x0 = 8 * (sg - r * SEGS);
            const uint8_t* dseg = dp + (r * DW + x0) * COS * 2 + d_lane;
            const uint8_t* aseg = ap + ((r + ky) * PW + x0) * CIS * 2;
            const h16x8 b1 = tr_frag(dseg, 4 * COS * 2), b2 = tr_frag(dseg + G::DZ_BYTES, 4 * COS * 2);
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const h16x8 a1 = tr_frag(aseg + a_lane[i], 4 * CIS * 2), a2 = tr_frag(aseg + a_lane[i] + G::A_BYTES, 4 * CIS * 2);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, b1, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b2, acc[i], 0, 0, 0);
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[i], 0, 0, 0);
            }
        }
    }
    const float inv = 1.0f / (sa * sd);
    const int co = os * COS + ntw * 32 + j;
    float* pp = part + (size_t)share * 25 * CI * CO;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = i * 32 + 8 * (r / 4) + 4 * h + (r % 4);            // accumulator r of lane (j, h) is row 8 (r / 4) + 4 h + r % 4
            const int kx = m / CIS, c = cs * CIS + m % CIS;
            if (kx < 5) pp[((size_t)(ky * 5 + kx) * CI + c) * CO + co] = acc[i][r] * inv;
        }
}

// sum of the partials in order -> gradient in the parameter layout [ci / CIC][tap][ci % CIC][co]
// (T = the taps of the convolution: 25, or 9 for the category network)
__global__ __launch_bounds__(256) void k_t_wgrad_reduce(const float* __restrict__ part, int nparts, int CI, int CO, int CIC, float* __restrict__ g, int T) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int total = T * CI * CO;
    if (idx >= total) return;
    const int co = idx % CO, cic = (idx / CO) % CIC, tap = (idx / (CO * CIC)) % T, cc = idx / (CO * CIC * T);
    const size_t src = ((size_t)tap * CI + cc * CIC + cic) * CO + co;
    float acc = 0.f;
    for (int p0 = 0; p0 < nparts; p0 += 8) {                            // eight loads in flight, added in part order
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p0 + k < nparts ? part[(size_t)(p0 + k) * total + src] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) if (p0 + k < nparts) acc += v[k];
    }
    g[idx] = acc;
}

// conv1 weight gradient (VALU): block = 8 rows of one crop -> part[block][c][tap][16].  Thread = (2 of the 8 rows, kernel row ky, output channel):
// per pixel one dz value and one new window value from LDS feed the five kx of the kernel row (a thread per tap read two LDS words per multiply
// and the kernel ran at the LDS rate); the four row pairs are added in order through LDS
template <int CH>
__global__ __launch_bounds__(512) void k_t_wgrad1(const float* __restrict__ x /*[n][80][80][CH]*/, const float* __restrict__ dz /*[n][80][80][16]*/,
                                                  float* __restrict__ part) {
    __shared__ float xs[12 * 84 * CH];
    __shared__ float ds[640 * 16];
    const int tid = threadIdx.x, crop = blockIdx.x / 10, row0 = (blockIdx.x % 10) * 8;
    for (int idx = tid; idx < 12 * 84 * CH; idx += 512) {
        const int c = idx % CH, px = (idx / CH) % 84, py = idx / (CH * 84);
        const int iy = row0 + py - 2, ix = px - 2;
        xs[idx] = (iy >= 0 && iy < 80 && ix >= 0 && ix < 80) ? x[(((size_t)crop * 80 + iy) * 80 + ix) * CH + c] : 0.f;
    }
    {
        const float4* src = reinterpret_cast<const float4*>(dz + ((size_t)crop * 80 + row0) * 80 * 16);
        for (int idx = tid; idx < 640 * 4; idx += 512) reinterpret_cast<float4*>(ds)[idx] = src[idx];
    }
    __syncthreads();
    const int co = tid & 15, ky = (tid >> 4) % 5, g = tid / 80;
    float acc[CH][5];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[c][k] = 0.f;
    if (tid < 320) {
#pragma unroll 1
        for (int yy = 0; yy < 2; ++yy) {
            const int y = g * 2 + yy;
            const float* xr = xs + (y + ky) * 84 * CH;
            const float* dr = ds + y * 80 * 16 + co;
            float win[CH][5];
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
                for (int k = 1; k < 5; ++k) win[c][k] = xr[(k - 1) * CH + c];
#pragma unroll 5
            for (int xx = 0; xx < 80; ++xx) {
                const float d = dr[xx * 16];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) win[c][k] = win[c][k + 1];
                    win[c][4] = xr[(xx + 4) * CH + c];
#pragma unroll
                    for (int k = 0; k < 5; ++k) acc[c][k] += win[c][k] * d;
                }
            }
        }
    }
    __syncthreads();                                                   // ds becomes the row pairs' exchange: [g][c][tap][co]
    if (tid < 320)
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int k = 0; k < 5; ++k) ds[((g * CH + c) * 25 + ky * 5 + k) * 16 + co] = acc[c][k];
    __syncthreads();
    if (tid >= 400) return;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        part[(size_t)blockIdx.x * CH * 400 + c * 400 + tid] = ((ds[c * 400 + tid] + ds[(CH + c) * 400 + tid]) + ds[(2 * CH + c) * 400 + tid]) + ds[(3 * CH + c) * 400 + tid];
}

// out[i] = sum over the parts, fixed order: 16 lanes per element take every 16th part, then the lane sums are added in order
__global__ __launch_bounds__(256) void k_t_reduce(const float* __restrict__ part, int nparts, int count, float* __restrict__ out) {
    __shared__ float sh[256];
    const int tid = threadIdx.x, e = tid & 15, ln = tid >> 4, idx = blockIdx.x * 16 + e;
    float acc = 0.f;
    if (idx < count) {
        for (int p0 = ln; p0 < nparts; p0 += 128) {                     // eight loads in flight, added in part order
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p0 + 16 * k < nparts ? part[(size_t)(p0 + 16 * k) * count + idx] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) if (p0 + 16 * k < nparts) acc += v[k];
        }
    }
    sh[ln * 16 + e] = acc;
    __syncthreads();
    if (tid < 16 && idx < count) {
        float r = 0.f;
        for (int k = 0; k < 16; ++k) r += sh[k * 16 + tid];
        out[idx] = r;
    }
}

// weights of the data-gradient convolutions: input channels = the forward layer's outputs, taps flipped.
// wb[cc'][t][cic'][co'] = w_fwd(ci = co', co = cc' * CICB + cic', tap = T - 1 - t); forward layout [ci / CIC][tap][ci % CIC][co]; T taps (25 or 9)
__global__ __launch_bounds__(256) void k_t_repack_bwd(const float* __restrict__ wf, int CI, int CO, int CIC, int COP /*padded output channels*/,
                                                      int CICB /*input-channel chunk of the data-gradient kernel*/, float* __restrict__ wb, int T) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int total = T * CO * COP;
    if (idx >= total) return;
    const int cop = idx % COP, cicp = (idx / COP) % CICB, t = (idx / (COP * CICB)) % T, ccp = idx / (COP * CICB * T);
    float v = 0.f;
    if (cop < CI) {
        const int ci = cop, co = ccp * CICB + cicp, tap = T - 1 - t;
        v = wf[(((size_t)(ci / CIC) * T + tap) * CIC + ci % CIC) * CO + co];
    }
    wb[idx] = v;
}

struct AdamSkip { uint32_t lo[6], hi[6]; };

// train() asserts 0 <= target < classes before it touches the model (visual_recognition_torch.py:1109-1112).  Targets handed over in device
// memory cannot be checked by the host without a synchronisation, so the step checks them first, on the device: refused[0] counts the steps
// that were refused -- this one if a target is out of range, and every following one until the host has reported the error (sticky) -- and
// the kernels that change the trainer's state (running statistics, Adam) return when it is set.  refused[1]: the same for an eval batch.
__global__ __launch_bounds__(256) void k_t_check_targets(const int32_t* __restrict__ targets, int n, int classes, int32_t* __restrict__ refused, int eval) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += 256) bad |= targets[i] < 0 || targets[i] >= classes;
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (eval) { if (s_bad) refused[1] = 1; }
        else if (s_bad || refused[0]) refused[0] += 1;
    }
}

// torch.optim.Adam (_single_tensor_adam, no weight decay / amsgrad): m.lerp_(g, 1 - b1); v = v * b2 + (1 - b2) g g;
// p += -step_size * m / (sqrt(v) / sqrt(bias_correction2) + eps)
__global__ __launch_bounds__(256) void k_t_adam(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M, float* __restrict__ V,
                                                uint32_t total, AdamSkip skip, float w1, float b2, float omb2, float step_size, float bc2_sqrt, float eps,
                                                const int32_t* __restrict__ refused) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total || *refused) return;                    // a refused step updates nothing
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (i >= skip.lo[k] && i < skip.hi[k]) return;          // running statistics are buffers, not parameters
    const float g = G[i];
    float m = M[i], v = V[i];
    m = m + w1 * (g - m);
    v = v * b2 + (omb2 * g) * g;
    M[i] = m; V[i] = v;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    P[i] = P[i] + (-step_size) * (m / denom);
}

__global__ __launch_bounds__(64) void k_t_loss(const float* __restrict__ loss, const int32_t* __restrict__ correct, int n, float* __restrict__ out /*[2]*/) {
    double s = 0;                                            // one wave: lane sums in index order, then a fixed butterfly
    int c = 0;
    for (int i = threadIdx.x; i < n; i += 64) { s += loss[i]; c += correct[i]; }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { s += __shfl_xor(s, d); c += __shfl_xor(c, d); }
    if (threadIdx.x == 0) { out[0] = (float)(s / n); out[1] = (float)c; }
}

// keep masks when the caller injects none: one counter-based hash per (step, layer, sample, channel)
__global__ __launch_bounds__(256) void k_t_masks(uint8_t* __restrict__ keep, size_t count, uint64_t seed, uint64_t step, float p_drop) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    uint64_t zed = seed + 0x9E3779B97F4A7C15ull * (step * 0x100000001B3ull + i + 1);
    zed = (zed ^ (zed >> 30)) * 0xBF58476D1CE4E5B9ull;
    zed = (zed ^ (zed >> 27)) * 0x94D049BB133111EBull;
    zed ^= zed >> 31;
    const float u = (float)(zed >> 40) * (1.0f / 16777216.0f);
    keep[i] = u >= p_drop ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// The 80x80 network as the host sees it (the kernels carry the same numbers as their own literals)
static constexpr int IMG = 80, IMG_PIX = IMG * IMG;                  // crop side; every block halves it: 80 -> 40 -> 20 -> 10
static constexpr int FC1_POS = (IMG / 8) * (IMG / 8), HID = 100;     // fc1: 100 positions x 128 channels -> 100 outputs
static constexpr int FC1_K = 128 * FC1_POS;                          // = 12800
// (keep masks of one step: four planes back to back, [n][16] [n][64] [n][128] (Dropout2d behind block 1..3) [n][100] (Dropout behind fc1);
// plane i starts at keep + n * tt.keep_off[i]: train_tensors.h)
static_assert(FC1_K == 12800 && T_COUNT == S_RM4 + 2, "fc1 of the 80x80 network; the slots of train_tensors.h are the blob's tensor ids");
static constexpr int C1_BPC = IMG / 4, WG1_BPC = IMG / 8;            // workgroups per crop of k_t_conv1 (4 rows each) and k_t_wgrad1 (8 rows)
static constexpr int RED_BLOCKS = T_RED_BLOCKS, BWD_BLOCKS = T_BWD_BLOCKS;   // grids of the reduction kernels (partials: red[BWD_BLOCKS][2][128])

// What each event of a step orders.  "main" is the context's stream, "side" the trainer's second one
enum {
    EV_PARAMS,       // main -> side: the side stream starts behind whatever wrote the parameters last
    EV_PACKED,       // side -> main: this step's fp16 weight images are packed (conv2 is the first to read them)
    EV_FORWARD,      // main -> side: the head has run (its gradients, fc1's weight gradient, the loss sum)
    EV_DZ3,          // main -> side: block i's dz is in z_i (bias finaliser, weight gradient)
    EV_DZ2,
    EV_DZ1,
    EV_SIDE_DONE,    // side -> main: the side stream's last piece of this step -- the join in front of Adam
    EV_MASKS,        // side -> main: this step's keep masks are drawn
    EV_COUNT
};

// A kernel instance that needs hipFuncAttributeMaxDynamicSharedMemorySize, bound to its geometry where it is named (trexhip_trainer_create):
// trainer_attrs and the launches read the same entry.  A convolution is one of three kernels (exactly one pointer is set)
struct ConvKernel {
    decltype(&k_conv5<16, 64, 40, 20, 16, CONV_EPI_RAW, 64>) f32 = nullptr;      // exact fp32 MFMA
    decltype(&k_conv5_n16<64, 40, 20, 16>) f32_n16 = nullptr;                    // ... 16 output channels on 16x16x4 tiles
    decltype(&k_t_conv5_h2<16, 64, 40, 20, 16, 64>) h2 = nullptr;                // fp16 two-piece split
    int lds = 0, bpc = 0;                                                        // dynamic LDS bytes, workgroups per crop
    int cic = 0, co = 0;                                                         // input-channel chunk and output-channel tile of its weight image
    const void* fn() const { return f32 ? reinterpret_cast<const void*>(f32) : f32_n16 ? reinterpret_cast<const void*>(f32_n16) : reinterpret_cast<const void*>(h2); }
};
template <int CI, int CO, int S, int ROWS, int CIC, int COUT>
static ConvKernel conv_f32() { using G = ConvGeom<CI, CO, S, ROWS, CIC>; return {&k_conv5<CI, CO, S, ROWS, CIC, CONV_EPI_RAW, COUT>, nullptr, nullptr, G::LDS_BYTES, G::BPC, CIC, CO}; }
template <int CI, int S, int ROWS, int CIC>
static ConvKernel conv_f32_n16() { using G = ConvGeom16<CI, S, ROWS, CIC>; return {nullptr, &k_conv5_n16<CI, S, ROWS, CIC>, nullptr, G::LDS_BYTES, G::BPC, CIC, 16}; }
template <int CI, int CO, int S, int ROWS, int CIC, int COUT>
static ConvKernel conv_h2() { using G = ConvGeomH<CI, CO, S, ROWS, CIC>; return {nullptr, nullptr, &k_t_conv5_h2<CI, CO, S, ROWS, CIC, COUT>, G::LDS_BYTES, G::BPC, CIC, CO}; }
// a weight gradient: grid = (block types, shares of the batch's work units), partials part[share][tap][ci][co]
struct WgradKernel {
    decltype(&k_t_wgrad<16, 64, 40, 16, 64, 3, 5>) fn = nullptr;                 // (k_t_wgrad_h2 has the same signature)
    int lds = 0, types = 0, units = 0 /*work units per crop*/, threads = 0, max_shares = 0;
};
template <int CI, int CO, int S, int CIS, int COS, int MT, int ROWS>
static WgradKernel wgrad_f32(int max_shares) { using G = WgradGeom<CI, CO, S, CIS, COS, MT, ROWS>; return {&k_t_wgrad<CI, CO, S, CIS, COS, MT, ROWS>, G::LDS_BYTES, G::TYPES, G::NB, 512, max_shares}; }
template <int CI, int CO, int S, int CIS, int ROWS>
static WgradKernel wgrad_h2(int max_shares) { using G = WgradHGeom<CI, CO, S, CIS, ROWS>; return {&k_t_wgrad_h2<CI, CO, S, CIS, ROWS>, G::LDS_BYTES, G::TYPES, G::NB, G::NTHR, max_shares}; }

// One convolution block [conv5x5 -> BatchNorm2d -> ReLU -> MaxPool2 -> Dropout2d], stated once (trexhip_trainer_create fills the three)
struct Layer {
    int C, CI;                             // output / input channels
    int ph, pw;                            // its plane: z [n][ph][pw][C], a and da [n][ph/2][pw/2][C] (the level's (h, w) of TrainAnyGeom: 80, 40, 20 at 80x80)
    int w, b, g, be, rm, rv;               // tensor ids: weight, bias, gamma, beta, running mean, running variance
    int dz_event;                          // recorded when its dz is complete
    int slot;                              // its statistics: stat + slot * 512 (mean, invstd, sums[2] x 128), red_bias + slot * BWD_BLOCKS * 128
    int keep_off;                          // its keep masks inside the mask row
    float *z = nullptr, *a = nullptr, *da = nullptr;
    // blocks 2 and 3: the three roles of its convolution at the trainer's precision, and the weight images they read
    ConvKernel fwd, dgrad;
    WgradKernel wgrad;
    int pack_blocks = 0;                   // grid of k_t_pack_h2
    uint4 *wh_f = nullptr, *wh_b = nullptr;   // precision 0: fp16 two-piece operand images (forward, data gradient) and their scale
    float* wh_scale = nullptr;
    float* wb = nullptr;                   // precision 1: flipped + transposed weights of the data gradient
};

// The streams of a step: main = the context's, w = the side stream (main itself when the step does not fork), es = main as events name it.
// Events go through the null stream when the caller's stream is the hipStreamLegacy handle (this runtime faults in a wait on an event
// recorded on the handle itself; in this library the two name the same stream); the per-thread handle has no such stand-in: the step then
// stays on the one stream
struct Streams { hipStream_t s, w, es; bool forked; };

struct Trainer : TrainerCore {
    bool any = false;                    // not 80x80: the convolutions of train_any.hip (exact fp32 whatever `precision` says)
    TrainAnyGeom geom{};                 // the planes and fc1's positions at every size; the convolutions' tiles and grids where `any`
    float* hsum = nullptr;               // any: fc1's partial planes added up (k_tany_fc1_sum), what the head reads as its one plane; 80x80: none, the head adds them
    Layer L[3] = {};
    decltype(&k_t_conv1<1>) conv1 = nullptr;      // block 1's convolution and weight gradient (no MFMA) at the trainer's 1 or 3 input channels
    decltype(&k_t_wgrad1<1>) wgrad1 = nullptr;
    float *part = nullptr /*conv2's / conv3's weight-gradient partials*/, *stat = nullptr /*3 x (mean, invstd, sums[2]) x 128*/;
    float *hpart = nullptr, *xhat = nullptr, *hd = nullptr, *dl = nullptr, *dy = nullptr, *dh = nullptr;
    double* red = nullptr;
    float* part1 = nullptr;              // conv1's weight-gradient partials (its kernels run beside the side stream's, which own `part`)
    // the training step forks: weight packing, the head's / fc1's / the convolutions' weight gradients and the loss sum run on `side`, beside the
    // chain that the next kernel waits for (data gradients, BN backward); the step joins again in front of Adam
    hipStream_t side = nullptr;
    hipEvent_t ev[EV_COUNT] = {};
    Streams q{};                         // the streams of the step being queued (begin_step)
    bool masks_on_side = false;          // this step's keep masks are being drawn on `side` (EV_MASKS)
    double* red_bias = nullptr;          // [3][BWD_BLOCKS][128]: k_tany_bn_bwd's column sums, finalized on `side`

    ~Trainer() override {
        if (side) (void)hipStreamSynchronize(side);                       // (a step joins its side stream before Adam; this is for a half-queued one)
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
    }
    const uint8_t* begin_step(hipStream_t s, int n, const uint8_t* injected) override;
    void forward(hipStream_t s, const float* x, const int32_t* targets, int n, const uint8_t* keep, bool train, float* probs) override;
    void backward(hipStream_t s, const float* x, int n, const uint8_t* keep) override;
    size_t blob_bytes() const override { return weight_blob_bytes(classes, CH, W, H); }
    void write_blob_header(void* blob) const override { write_weight_blob_header(blob, classes, W, H, CH); }
};

// every kernel instance of the table that needs more dynamic LDS than the default limit
static int trainer_attrs(Trainer* t) {
    for (const Layer& L : t->L) {
        for (const ConvKernel* k : {&L.fwd, &L.dgrad})
            if (k->fn()) TH_CHECK_HIP(hipFuncSetAttribute(k->fn(), hipFuncAttributeMaxDynamicSharedMemorySize, k->lds));
        if (L.wgrad.fn) TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(L.wgrad.fn), hipFuncAttributeMaxDynamicSharedMemorySize, L.wgrad.lds));
    }
    return TREXHIP_OK;
}

// z -> a.  train: batch statistics (from the `partials` column sums the convolution's workgroups left in t->red, or from a pass of its own
// over z when there are none) + dropout masks; eval: running statistics (the caller's masks keep everything)
static void bn_forward(Trainer* t, hipStream_t s, const Layer& L, int n, const uint8_t* keep, float scale, bool train, int partials) {
    float* P = t->P;
    const size_t* o = t->tt.off;
    float* mean = t->stat + L.slot * 512;
    float* invstd = mean + 128;
    if (train) {
        const size_t rows = (size_t)n * L.ph * L.pw;                  // every pixel counts in the statistics, the odd last row / column too
        if (!partials) t_bn_stats(s, L.C, L.z, rows, t->red);
        hipLaunchKernelGGL((k_t_red_finalize<FIN_BN_STATS>), dim3(L.C), dim3(256), 0, s, t->red, partials ? partials : RED_BLOCKS, L.C,
                           FinArgs{(double)rows, t->p.bn_momentum, mean, invstd, P + o[L.rm], P + o[L.rv], t->bad_target});
    } else {
        hipLaunchKernelGGL(k_t_bn_from_running, dim3(1), dim3(128), 0, s, P + o[L.rm], P + o[L.rv], L.C, mean, invstd);
    }
    tany_bn_pool(s, L.C, L.z, mean, invstd, P + o[L.g], P + o[L.be], keep + (size_t)n * L.keep_off, scale, L.a, n, L.ph, L.pw);
}

// da (pooled gradient) -> dz written over z; gradients of gamma and beta.  Returns the grid of k_tany_bn_bwd, whose column sums bias_finalize adds
static int bn_backward(Trainer* t, hipStream_t s, const Layer& L, int n, const uint8_t* keep, float scale) {
    float* P = t->P;
    const size_t* o = t->tt.off;
    float* mean = t->stat + L.slot * 512;
    float* invstd = mean + 128;
    float* sums = mean + 256;
    const uint8_t* kp = keep + (size_t)n * L.keep_off;
    tany_pool_bwd_stats(s, L.C, RED_BLOCKS, L.da, L.z, mean, invstd, P + o[L.g], P + o[L.be], kp, scale, n, L.ph, L.pw, t->red);
    hipLaunchKernelGGL((k_t_red_finalize<FIN_BN_BWD>), dim3(L.C), dim3(256), 0, s, t->red, RED_BLOCKS, L.C,
                       FinArgs{0.0, 0.f, sums, t->G + o[L.g], t->G + o[L.be], nullptr, nullptr});
    const float inv_count = (float)(1.0 / ((double)n * L.ph * L.pw));      // the means run over every pixel of the plane
    return tany_bn_bwd(s, L.C, BWD_BLOCKS, L.da, L.z, mean, invstd, P + o[L.g], P + o[L.be], kp, scale, sums, inv_count, n, L.ph, L.pw,
                       t->red_bias + (size_t)L.slot * BWD_BLOCKS * 128);
}
// the convolution bias's gradient from k_tany_bn_bwd's column sums (nothing but Adam waits for it: the caller puts it on the side stream)
static void bias_finalize(Trainer* t, hipStream_t w, const Layer& L, int nb) {
    hipLaunchKernelGGL((k_t_red_finalize<FIN_BIAS>), dim3(L.C), dim3(256), 0, w, t->red_bias + (size_t)L.slot * BWD_BLOCKS * 128, nb, L.C,
                       FinArgs{0.0, 0.f, t->G + t->tt.off[L.b], nullptr, nullptr, nullptr, nullptr});
}

static void fork(Trainer* t, const Streams& q, int e) {
    if (q.forked) { (void)hipEventRecord(t->ev[e], q.es); (void)hipStreamWaitEvent(q.w, t->ev[e], 0); }
}

// One block backwards: dz on the main stream; behind it the side stream takes the bias gradient and the weight gradient with its reduce
// (nothing but Adam waits for them) while the main stream goes on with the data gradient, which the block below waits for.  Block 1 ends
// behind the bias: it has no data gradient, and the caller runs its weight gradient
static void block_backward(Trainer* t, const Streams& q, const Layer& L, int n, const uint8_t* keep, float scale) {
    const int nb = bn_backward(t, q.s, L, n, keep, scale);
    fork(t, q, L.dz_event);
    bias_finalize(t, q.w, L, nb);
    if (L.slot == 0) return;
    const Layer& below = t->L[L.slot - 1];
    if (t->any) {
        const int shares = t->geom.wg_shares(L.slot, n);
        tany_wgrad(q.w, t->geom, L.slot, n, below.a, L.z, t->part);
        hipLaunchKernelGGL(k_t_wgrad_reduce, dim3((25 * L.CI * L.C + 255) / 256), dim3(256), 0, q.w, t->part, shares, L.CI, L.C, L.fwd.cic, t->G + t->tt.off[L.w], 25);
        hipLaunchKernelGGL(k_t_repack_bwd, dim3((25 * L.C * L.dgrad.co + 255) / 256), dim3(256), 0, q.s, t->P + t->tt.off[L.w], L.CI, L.C, L.fwd.cic, L.dgrad.co, L.dgrad.cic, L.wb, 25);
        tany_conv_dgrad(q.s, t->geom, L.slot, n, L.z, L.wb, below.da);
        return;
    }
    const WgradKernel& g = L.wgrad;
    const int shares = std::min(n * g.units, g.max_shares);
    hipLaunchKernelGGL(g.fn, dim3(g.types, shares), dim3(g.threads), g.lds, q.w, below.a, L.z, t->part, n);
    hipLaunchKernelGGL(k_t_wgrad_reduce, dim3((25 * L.CI * L.C + 255) / 256), dim3(256), 0, q.w, t->part, shares, L.CI, L.C, L.fwd.cic, t->G + t->tt.off[L.w], 25);
    // the data gradient: the same convolution on flipped + transposed weights
    const ConvKernel& k = L.dgrad;
    if (!k.h2) hipLaunchKernelGGL(k_t_repack_bwd, dim3((25 * L.C * k.co + 255) / 256), dim3(256), 0, q.s, t->P + t->tt.off[L.w], L.CI, L.C, L.fwd.cic, k.co, k.cic, L.wb, 25);
    if (k.h2) hipLaunchKernelGGL(k.h2, dim3(n * k.bpc), dim3(512), k.lds, q.s, L.z, L.wh_b, nullptr, below.da, L.wh_scale, nullptr);
    else if (k.f32_n16) hipLaunchKernelGGL(k.f32_n16, dim3(n * k.bpc), dim3(512), k.lds, q.s, L.z, L.wb, below.da);
    else hipLaunchKernelGGL(k.f32, dim3(n * k.bpc), dim3(512), k.lds, q.s, L.z, L.wb, nullptr, below.da);
}

// forward pass up to the per-sample loss / arg-max (and, as a by-product of k_t_head, the gradient at the fc1 output).  train = batch
// statistics + dropout masks `keep`; eval = running statistics, nothing dropped (model.eval(), visual_recognition_torch.py:1171-1185).
// probs (eval only): the head writes the softmax rows there and nothing else (k_t_head_eval)
void Trainer::forward(hipStream_t s, const float* x, const int32_t* targets, int n, const uint8_t* keep, bool train, float* probs) {
    Trainer* t = this;
    const float scale = train ? 1.0f / (1.0f - p.dropout) : 1.0f;
    hipStream_t side = train && q.forked ? q.w : nullptr;             // a training step packs its weights beside conv1
    float* P = t->P;
    const size_t* o = t->tt.off;
    const Layer* L = t->L;
    const bool h2 = t->p.precision == 0 && !t->any;
    hipStream_t es = s == hipStreamLegacy ? nullptr : s;
    if (h2) {
        // this step's weights as fp16 two-piece operand images (both directions); conv2 is the first to need them
        for (int i = 1; i < 3; ++i)
            hipLaunchKernelGGL(k_t_pack_h2, dim3(L[i].pack_blocks), dim3(1024), 0, side ? side : s, P + o[L[i].w], L[i].CI, L[i].C, L[i].fwd.cic, L[i].fwd.cic,
                               L[i].dgrad.cic, L[i].dgrad.co, L[i].wh_f, L[i].wh_b, L[i].wh_scale);
        if (side) (void)hipEventRecord(t->ev[EV_PACKED], side);
    }
    if (t->any) tany_conv1(s, t->geom, n, x, P + o[T_C1W], P + o[T_C1B], L[0].z);
    else hipLaunchKernelGGL(t->conv1, dim3(n * C1_BPC), dim3(320), 0, s, x, P + o[T_C1W], P + o[T_C1B], L[0].z, train ? t->red : nullptr);
    if (side && t->masks_on_side) (void)hipStreamWaitEvent(es, t->ev[EV_MASKS], 0);
    bn_forward(t, s, L[0], n, keep, scale, train, t->any ? 0 : n * C1_BPC);      // (any: no column sums from the convolution, k_t_bn_stats reads z)
    if (h2 && side) (void)hipStreamWaitEvent(es, t->ev[EV_PACKED], 0);
    for (int i = 1; i < 3; ++i) {
        const ConvKernel& k = L[i].fwd;                              // the fp16 kernel leaves its BN column sums, the fp32 one does not
        if (t->any) tany_conv_fwd(s, t->geom, i, n, L[i - 1].a, P + o[L[i].w], P + o[L[i].b], L[i].z);
        else if (k.h2) hipLaunchKernelGGL(k.h2, dim3(n * k.bpc), dim3(512), k.lds, s, L[i - 1].a, L[i].wh_f, P + o[L[i].b], L[i].z, L[i].wh_scale, train ? t->red : nullptr);
        else hipLaunchKernelGGL(k.f32, dim3(n * k.bpc), dim3(512), k.lds, s, L[i - 1].a, P + o[L[i].w], P + o[L[i].b], L[i].z);
        bn_forward(t, s, L[i], n, keep, scale, train, k.h2 ? n * k.bpc : 0);
    }
    tany_fc1(s, t->geom, n, L[2].a, P + o[T_F1W], t->hpart, t->hsum);         // (80x80: no hsum and no launch for it -- the head adds the 100 planes)
    const float* planes = t->any ? t->hsum : t->hpart;
    if (probs) {
        hipLaunchKernelGGL(t->any ? &k_t_head_eval<1> : &k_t_head_eval<FC1_POS>, dim3(n), dim3(128), 0, s, planes, n, P + o[T_F1B], P + o[T_LNG], P + o[T_LNB], P + o[T_F2W], P + o[T_F2B], t->classes, probs);
        return;
    }
    hipLaunchKernelGGL(t->any ? &k_t_head<1> : &k_t_head<FC1_POS>, dim3(n), dim3(128), 0, s, planes, n, P + o[T_F1B], P + o[T_LNG], P + o[T_LNB], keep + (size_t)n * tt.keep_off[3], scale, P + o[T_F2W],
                       P + o[T_F2B], targets, t->classes, t->xhat, t->hd, t->dl, t->dy, t->dh, t->loss, t->correct, t->bad_target);
}

// a step starts by forking: the side stream waits for whatever wrote the parameters last, then draws the masks beside conv1
const uint8_t* Trainer::begin_step(hipStream_t s, int n, const uint8_t* injected) {
    const bool forked = s != hipStreamPerThread;
    q = Streams{s, forked ? side : s, s == hipStreamLegacy ? nullptr : s, forked};
    fork(this, q, EV_PARAMS);
    masks_on_side = forked && !injected;
    if (injected) return injected;
    const size_t count = (size_t)n * tt.keep_row;
    hipLaunchKernelGGL(k_t_masks, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, q.w, keep, count, p.seed, (uint64_t)step, p.dropout);
    if (forked) (void)hipEventRecord(ev[EV_MASKS], q.w);
    return keep;
}

void Trainer::backward(hipStream_t s, const float* x, int n, const uint8_t* keep) {
    Trainer* t = this;
    const float scale = 1.0f / (1.0f - p.dropout);
    float* P = t->P;
    float* G = t->G;
    const size_t* o = tt.off;
    const bool forked = q.forked;
    hipStream_t w = q.w;
    fork(t, q, EV_FORWARD);
    {
        const int cnt = t->classes * HID + t->classes + 3 * HID;
        hipLaunchKernelGGL(k_t_head_grads, dim3((cnt + 255) / 256), dim3(256), 0, w, t->dl, t->hd, t->dy, t->xhat, t->dh, n, t->classes, G + o[T_F2W], G + o[T_F2B],
                           G + o[T_LNG], G + o[T_LNB], G + o[T_F1B]);
    }
    tany_fc1_wgrad(w, t->geom, n, t->L[2].a, t->dh, G + o[T_F1W]);
    hipLaunchKernelGGL(k_t_loss, dim3(1), dim3(64), 0, w, t->loss, t->correct, n, t->out2);
    tany_fc1_dgrad(s, t->geom, n, t->dh, P + o[T_F1W], t->L[2].da);
    for (int i = 2; i >= 0; --i) block_backward(t, q, t->L[i], n, keep, scale);
    if (forked) (void)hipEventRecord(t->ev[EV_SIDE_DONE], w);               // the side stream's last piece of this step
    if (t->any) tany_wgrad1(s, t->geom, n, x, t->L[0].z, t->part1);
    else hipLaunchKernelGGL(t->wgrad1, dim3(n * WG1_BPC), dim3(512), 0, s, x, t->L[0].z, t->part1);
    hipLaunchKernelGGL(k_t_reduce, dim3((t->CH * 400 + 15) / 16), dim3(256), 0, s, t->part1, n * (t->any ? t->geom.wg1_tiles : WG1_BPC), t->CH * 400, G + o[T_C1W]);
    if (forked) (void)hipStreamWaitEvent(q.es, t->ev[EV_SIDE_DONE], 0);     // join: every gradient is in G
}

// ------------------------------------------------------------------------------------------------
// train_host.h: the size-independent kernels as the core (train_host.hip) and the one-stream chain (train_arch.hip) launch them
// ------------------------------------------------------------------------------------------------
void t_bn_stats(hipStream_t s, int C, const float* d, size_t rows, double* partial) {
    const auto fn = C == 16 ? &k_t_bn_stats<16> : C == 64 ? &k_t_bn_stats<64> : &k_t_bn_stats<128>;
    hipLaunchKernelGGL(fn, dim3(RED_BLOCKS), dim3(256), 0, s, d, rows, partial);
}
void t_fin_bn_stats(hipStream_t s, const double* partial, int nblocks, int C, double count, float momentum, float* mean, float* invstd, float* run_mean,
                    float* run_var, const int32_t* refused) {
    hipLaunchKernelGGL((k_t_red_finalize<FIN_BN_STATS>), dim3(C), dim3(256), 0, s, partial, nblocks, C, FinArgs{count, momentum, mean, invstd, run_mean, run_var, refused});
}
void t_fin_bn_bwd(hipStream_t s, const double* partial, int nblocks, int C, float* sums, float* d_gamma, float* d_beta) {
    hipLaunchKernelGGL((k_t_red_finalize<FIN_BN_BWD>), dim3(C), dim3(256), 0, s, partial, nblocks, C, FinArgs{0.0, 0.f, sums, d_gamma, d_beta, nullptr, nullptr});
}
void t_fin_bias(hipStream_t s, const double* partial, int nblocks, int C, float* d_bias) {
    hipLaunchKernelGGL((k_t_red_finalize<FIN_BIAS>), dim3(C), dim3(256), 0, s, partial, nblocks, C, FinArgs{0.0, 0.f, d_bias, nullptr, nullptr, nullptr, nullptr});
}
void t_bn_from_running(hipStream_t s, const float* run_mean, const float* run_var, int C, float* mean, float* invstd) {
    hipLaunchKernelGGL(k_t_bn_from_running, dim3(1), dim3(128), 0, s, run_mean, run_var, C, mean, invstd);
}
void t_wgrad_reduce(hipStream_t s, const float* part, int shares, int CI, int CO, int CIC, float* g, int taps) {
    hipLaunchKernelGGL(k_t_wgrad_reduce, dim3((taps * taps * CI * CO + 255) / 256), dim3(256), 0, s, part, shares, CI, CO, CIC, g, taps * taps);
}
void t_reduce(hipStream_t s, const float* part, int nparts, int count, float* out) {
    hipLaunchKernelGGL(k_t_reduce, dim3((count + 15) / 16), dim3(256), 0, s, part, nparts, count, out);
}
void t_repack_bwd(hipStream_t s, const float* wf, int CI, int CO, int CIC, int COP, int CICB, float* wb, int taps) {
    hipLaunchKernelGGL(k_t_repack_bwd, dim3((taps * taps * CO * COP + 255) / 256), dim3(256), 0, s, wf, CI, CO, CIC, COP, CICB, wb, taps * taps);
}
void t_adam(hipStream_t s, float* P, const float* G, float* M, float* V, size_t total, const uint32_t* skip_lo, const uint32_t* skip_hi, int nskip, double lr,
            double beta1, double beta2, float eps, int64_t step, const int32_t* refused) {
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamSkip skip{};
    for (int k = 0; k < nskip && k < 6; ++k) { skip.lo[k] = skip_lo[k]; skip.hi[k] = skip_hi[k]; }
    hipLaunchKernelGGL(k_t_adam, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, P, G, M, V, (uint32_t)total, skip, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)(lr / bc1), (float)std::sqrt(bc2), eps, refused);
}
void t_masks(hipStream_t s, uint8_t* keep, size_t count, uint64_t seed, uint64_t step, float p_drop) {
    hipLaunchKernelGGL(k_t_masks, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, keep, count, seed, step, p_drop);
}
void t_check_targets(hipStream_t s, const int32_t* targets, int n, int classes, int32_t* refused, int eval) {
    hipLaunchKernelGGL(k_t_check_targets, dim3(1), dim3(256), 0, s, targets, n, classes, refused, eval);
}
void t_loss(hipStream_t s, const float* loss, const int32_t* correct, int n, float* out2) {
    hipLaunchKernelGGL(k_t_loss, dim3(1), dim3(64), 0, s, loss, correct, n, out2);
}

// a V118_3 blob (parse_weight_blob refuses every other identity network: none of those trains here)
int v118_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, TrainerCore** out) {
    WeightBlob wb;
    const int prc = parse_weight_blob(blob, bytes, "trexhip_trainer_create", &wb, [](int W, int H) -> int {
        if (W < 8 || W > 256 || H < 8 || H > 256) {               // the range of trexhip_load_weights
            set_error("trexhip_trainer_create: individual_image_size " + std::to_string(W) + "x" + std::to_string(H) + " is outside 8..256 x 8..256");
            return TREXHIP_E_UNSUPPORTED;
        }
        return TREXHIP_OK;
    });
    if (prc != TREXHIP_OK) return prc;
    const int classes = wb.classes, CH = wb.CH;
    if (const int rc = check_train_params(p)) return rc;
    if (hipSetDevice(ctx->p.device) != hipSuccess) { set_error("trexhip_trainer_create: hipSetDevice failed"); return TREXHIP_E_DEVICE; }
    Trainer* t = new Trainer();
    t->ctx = ctx; t->version = TREXHIP_NET_V118_3; t->classes = classes; t->CH = CH; t->max_n = p->max_batch; t->p = *p;
    t->W = wb.W; t->H = wb.H;
    t->tt = train_tensors(TRAIN_V118_3, wb.W, wb.H, CH, classes);
    t->any = wb.W != IMG || wb.H != IMG;
    t->geom = train_any_geom(wb.W, wb.H, CH);
    // ---- the three blocks and their kernel instances.  The convolutions' precision is chosen here, once per role
    const bool h2 = p->precision == 0 && !t->any;      // every other size runs the exact-fp32 chain at both precisions
    Layer* L = t->L;
    const TrainAnyLayer* gl = t->geom.L;
    //      C    CI  plane           weight bias   gamma beta   running mean / variance  dz event  slot  masks
    L[0] = {16,  CH, gl[0].h, gl[0].w, T_C1W, T_C1B, T_G1, T_BE1, T_RM1, T_RV1, EV_DZ1, 0, (int)t->tt.keep_off[0]};
    L[1] = {64,  16, gl[1].h, gl[1].w, T_C2W, T_C2B, T_G2, T_BE2, T_RM2, T_RV2, EV_DZ2, 1, (int)t->tt.keep_off[1]};
    L[2] = {128, 64, gl[2].h, gl[2].w, T_C3W, T_C3B, T_G3, T_BE3, T_RM3, T_RV3, EV_DZ3, 2, (int)t->tt.keep_off[2]};
    if (t->any) {
        // the generic convolutions (train_any.hip) follow t->geom in their three roles; what the shared kernels (k_t_wgrad_reduce, k_t_repack_bwd)
        // read of a convolution is its weight image: the parameter layout's chunk, the data gradient's chunk and tile
        L[1].fwd.cic = 16; L[1].dgrad.cic = 16; L[1].dgrad.co = 32;        // conv2's data gradient: 16 real channels in a 32-wide tile
        L[2].fwd.cic = 32; L[2].dgrad.cic = 32; L[2].dgrad.co = 64;
    } else {
        t->conv1 = CH == 1 ? &k_t_conv1<1> : &k_t_conv1<3>;
        t->wgrad1 = CH == 1 ? &k_t_wgrad1<1> : &k_t_wgrad1<3>;
        // conv3 forward in 10-row bands: 2 blocks per crop (a training batch is 64..128 crops, the chip has 256 CUs; 4-row bands measured no faster).
        // conv2's data gradient has 16 output channels: 16x16x4 tiles in fp32, 16 of a 32-wide tile's channels real in fp16
        L[1].fwd = h2 ? conv_h2<16, 64, 40, 20, 16, 64>() : conv_f32<16, 64, 40, 20, 16, 64>();
        L[2].fwd = h2 ? conv_h2<64, 128, 20, 10, 32, 128>() : conv_f32<64, 128, 20, 10, 32, 128>();
        L[1].dgrad = h2 ? conv_h2<64, 32, 40, 20, 16, 16>() : conv_f32_n16<64, 40, 20, 16>();
        L[2].dgrad = h2 ? conv_h2<128, 64, 20, 10, 32, 64>() : conv_f32<128, 64, 20, 10, 32, 64>();
        // weight gradients.  fp32: conv2 block type = kernel row (5 types), unit = 5 rows of a crop; conv3 block type = kernel row x 32-channel half x
        // 64-channel half (20 types), unit = 10 rows; 5 x 51 = 255 and 20 x 12 = 240 workgroups: one round on 256 CUs.  fp16: conv2 1 type x 256 shares,
        // conv3 4 x 64
        L[1].wgrad = h2 ? wgrad_h2<16, 64, 40, 16, 10>(256) : wgrad_f32<16, 64, 40, 16, 64, 3, 5>(51);
        L[2].wgrad = h2 ? wgrad_h2<64, 128, 20, 32, 10>(64) : wgrad_f32<64, 128, 20, 32, 64, 5, 10>(12);
        L[1].pack_blocks = 10; L[2].pack_blocks = 50;
    }
    // ---- memory
    const size_t n = (size_t)t->max_n;
    int rc = TREXHIP_OK;
    const char* who = "trexhip_trainer_create";
#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)
    size_t part_floats = t->any ? t->geom.part_floats() : 0;
    for (int i = 0; i < 3; ++i) {
        const size_t act = n * L[i].ph * L[i].pw * L[i].C;                      // z; pooled: a quarter of it at 80x80, the floored plane elsewhere
        const size_t pooled = n * (L[i].ph / 2) * (L[i].pw / 2) * L[i].C;
        TRY(t->mem.device(&L[i].z, act, who)); TRY(t->mem.device(&L[i].a, pooled, who)); TRY(t->mem.device(&L[i].da, pooled, who));
        part_floats = std::max(part_floats, (size_t)L[i].wgrad.max_shares * 25 * L[i].CI * L[i].C);
    }
    if (h2) {                                                                 // the weight images of the trainer's own precision
        TRY(t->mem.device(&L[1].wh_f, (size_t)2 * 2 * 25 * 64, who)); TRY(t->mem.device(&L[1].wh_b, (size_t)2 * 8 * 25 * 32, who));
        TRY(t->mem.device(&L[2].wh_f, (size_t)2 * 8 * 25 * 128, who)); TRY(t->mem.device(&L[2].wh_b, (size_t)2 * 16 * 25 * 64, who));
        TRY(t->mem.device(&L[1].wh_scale, 2, who));
        L[2].wh_scale = L[1].wh_scale + 1;
    } else {
        TRY(t->mem.device(&L[2].wb, (size_t)4 * 25 * 32 * 64, who)); TRY(t->mem.device(&L[1].wb, (size_t)2 * 25 * 32 * 32, who));
    }
    TRY(t->mem.device(&t->part, part_floats, who)); TRY(t->mem.device(&t->part1, t->any ? t->geom.part1_floats(n) : n * WG1_BPC * CH * 400, who)); TRY(t->mem.device(&t->red_bias, (size_t)3 * BWD_BLOCKS * 128, who));
    TRY(t->mem.device(&t->stat, (size_t)3 * 512, who));
    TRY(t->mem.device(&t->hpart, n * t->geom.P * HID, who)); if (t->any) TRY(t->mem.device(&t->hsum, n * HID, who)); TRY(t->mem.device(&t->xhat, n * HID, who)); TRY(t->mem.device(&t->hd, n * HID, who));
    TRY(t->mem.device(&t->dl, n * classes, who)); TRY(t->mem.device(&t->dy, n * HID, who)); TRY(t->mem.device(&t->dh, n * HID, who));
    TRY(t->mem.device(&t->red, std::max((size_t)BWD_BLOCKS * 2 * 128, n * 640), who));   // conv1 leaves 20 n x 2 x 16 partials, conv2 / conv3 2 n x 2 x C
    if (rc == TREXHIP_OK && hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking) != hipSuccess) { set_error("trexhip_trainer_create: no second stream"); rc = TREXHIP_E_DEVICE; }
    for (hipEvent_t& e : t->ev)
        if (rc == TREXHIP_OK && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { set_error("trexhip_trainer_create: no event"); rc = TREXHIP_E_DEVICE; }
    TRY(trainer_attrs(t));
    if (t->any) TRY(tany_attrs());
    TRY(t->init_state(wb.t, who));
#undef TRY
    if (rc != TREXHIP_OK) { delete t; return rc; }
    *out = t;
    return TREXHIP_OK;
}

}  // namespace trexhip

extern "C" size_t trexhip_weight_blob_bytes(int32_t classes, int32_t channels) { return trexhip::weight_blob_bytes(classes, channels, trexhip::IMG, trexhip::IMG); }
