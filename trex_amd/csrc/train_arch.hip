// train_arch.hip -- the training step of the networks that run the generic chain on one stream: the identity networks v100 and v110
// (visual_identification_network_torch.py:262-382, train mode; the loop body visual_recognition_torch.py:1137-1158) and the category network
// (trex_learn_category.py:18-44, PyTorchModel, in train mode; the loop body :314-332 on a non-CUDA device: fp32 arithmetic.  On `cuda` the reference
// adds autocast and a GradScaler; that arithmetic is not restated), at every size they load: W, H = 8..256, CH = 1 or 3, NHWC fp32, exact fp32
// arithmetic at both values of trexhip_train_params.precision.
//
//   v100      [conv5x5 'same' -> ReLU -> MaxPool2 -> Dropout2d(0.25)] x3 -> flatten (NCHW) -> fc1 -> ReLU -> Dropout(0.5) -> fc2 -> cross entropy
//   v110      [conv5x5 'same' -> MaxPool2 -> BatchNorm2d -> ReLU -> Dropout2d(0.25)] x3 -> flatten -> fc1 -> BatchNorm1d -> ReLU -> Dropout(0.25) -> fc2
//   category  x = byte / 127.5 - 1, zero padded -> [conv3x3 pad 1 -> BatchNorm2d -> ReLU -> MaxPool2 -> Dropout(0.25)] x3 (16, 64, 100 channels)
//             -> flatten -> fc1 (100) -> ReLU -> Dropout(0.25) -> fc2 (categories); nn.Dropout on [n][C][h/2][w/2]: ELEMENT-wise keep masks
//
// One trainer type, ChainTrainer (the host side at the end of this file), runs all three: it derives from TrainerCore (train_host.h) and a network is
// a row of data plus the functions of its block kind and its head.  The category network adds no kernel: its blocks are train_any.hip's block kernels
// (tany_bn_pool, tany_pool_bwd_stats, tany_bn_bwd) with `creal`, its convolutions the 3-tap mode of the same chain, its head v100's; BatchNorm's
// statistics run over all n h w pixels of the convolution's plane, the odd last row and column included, and block 3's plane has at least 2 x 2 pixels
// at every legal size, so n = 1 trains.
// The convolutions are V118_3's with conv3 at 100 outputs instead of 128, so the three roles of every convolution, both conv1 kernels and fc1 are
// train_any.hip's (tany_*), and the reductions, Adam, the masks, the target check and the loss sum train.hip's (t_*, train_host.h).  The 100 channels
// travel padded to 128 in z3, a3, their gradients and the packed images of conv3.weight and fc1.weight; every per-channel tensor of block 3 has
// 128 slots.  A padded slot holds 0 and stays 0: its weights and bias are 0, so z = 0; the kernels below give a channel >= 100 the activation 0
// and the gradient 0 whatever its slots hold, so the weight gradients' padded columns and fc1's padded rows are sums of zeros, and Adam's update of
// (p, g, m, v) = 0 is 0.  trexhip_trainer_read and the exported blob walk torch's 100.
//
// What is new here is what lies around the convolutions:
//   k_tarch_pool<C, V100>           v110: p = floor 2x2 max of the raw z and the arg-max (first maximum in row-major order) as one byte per
//                                   (window, channel); v100: a = dropout(max(0, max z)) and the byte (4 = the gate is closed)
//   k_t_bn_stats + k_t_red_finalize on the n (h/2)(w/2) pooled rows: the dropped odd row / column of z is in no statistic
//   k_tarch_bn_apply<C>             a = dropout(relu(gamma x-hat + beta)); eval: running statistics
//   k_tarch_bn_bwd_stats<C>         sum dy, sum dy x-hat over the pooled rows, dy = da keep scale [y > 0]
//   k_tarch_unpool<C, V100>         dp = gamma invstd (dy - mean dy - x-hat mean(dy x-hat)) (v100: dp = da scale), dz = dp at the window's byte, 0 at the
//                                   other three pixels and in the dropped odd row / column, written over z; the column sums are the conv bias's gradient
//   k_tarch_bn1d_stats, k_tarch_head<BN>, k_tarch_bn1d_sums, k_tarch_bn1d_dh, k_tarch_head_grads       the two heads
// The arg-max is stored, not recomputed: the backward pass then never reads z (16 B per window and channel) for 1 B written and 1 B read.
// Every sum has a fixed order that depends on the size and n alone; no floating-point atomics, no tickets.  One stream: nothing forks.
#include "internal.h"
#include "cnn_weights.h"
#include "train_dev.h"
#include "train_any.h"
#include "train_host.h"
#include "train_arch.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace trexhip {
namespace {

constexpr float EPS_BN = 1e-5f;
constexpr int HID = TA_HID;

// the BatchNorm output of one element, the one expression forward and backward share (the ReLU gate is [y > 0] of this value on both ways)
__device__ __forceinline__ float bn_y(const float xhat, const float gamma, const float beta) { return xhat * gamma + beta; }

template <int C>
__device__ __forceinline__ void load_window(const float* __restrict__ z, int H, int W, int crop, int py, int px, int c4, float4 v[4]) {
    const float* base = z + (((size_t)crop * H + 2 * py) * W + 2 * px) * C + c4 * 4;
    v[0] = *reinterpret_cast<const float4*>(base);
    v[1] = *reinterpret_cast<const float4*>(base + C);
    v[2] = *reinterpret_cast<const float4*>(base + (size_t)W * C);
    v[3] = *reinterpret_cast<const float4*>(base + (size_t)W * C + C);
}

// ------------------------------------------------------------------------------------------------
// floor 2x2 max-pool of the raw convolution output: z [n][H][W][C] -> out [n][H/2][W/2][C] and arg [n][H/2][W/2][C] bytes (one 32-bit store per
// lane).  The arg-max is the first maximum in row-major order, like torch's max_pool2d.  V100: out = dropout(relu(max)), the byte is 4 where no
// gradient passes (max <= 0, a dropped or a padded channel); v110: out = the raw maximum.  The odd last row / column is read by no window
// ------------------------------------------------------------------------------------------------
template <int C, bool V100>
__global__ __launch_bounds__(256) void k_tarch_pool(const float* __restrict__ z, const uint8_t* __restrict__ keep /*[n][creal], V100*/, const int creal,
                                                    const float scale, float* __restrict__ out, uint32_t* __restrict__ arg4, const int n, const int H, const int W) {
    const int Hp = H / 2, Wp = W / 2;
    const size_t total = (size_t)n * Hp * Wp * (C / 4);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = idx % (C / 4);
    const size_t pos = idx / (C / 4);
    const int px = pos % Wp, py = (pos / Wp) % Hp, crop = pos / ((size_t)Hp * Wp);
    float4 v[4];
    load_window<C>(z, H, W, crop, py, px, c4, v);
    float4 o;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float best = f4get(v[0], k);
        uint32_t bi = 0;
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const float t = f4get(v[q], k);
            if (t > best) { best = t; bi = q; }
        }
        if (V100) {
            const int c = c4 * 4 + k;
            const bool open = c < creal && keep[(size_t)crop * creal + c] != 0 && best > 0.f;
            f4set(o, k, open ? best * scale : 0.f);
            if (!open) bi = 4;
        } else {
            f4set(o, k, best);
        }
        packed |= bi << (8 * k);
    }
    *reinterpret_cast<float4*>(out + pos * C + c4 * 4) = o;
    arg4[pos * (C / 4) + c4] = packed;
}

// ------------------------------------------------------------------------------------------------
// v110: BatchNorm2d + ReLU + Dropout2d on the pooled plane: p [rows][C] -> a [rows][C], rows = n * hw.  A channel >= creal gives 0
// ------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void k_tarch_bn_apply(const float* __restrict__ p, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ g, const float* __restrict__ be, const uint8_t* __restrict__ keep /*[n][creal]*/,
                                                        const int creal, const float scale, float* __restrict__ a, const size_t rows, const int hw) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * (C / 4)) return;
    const int c4 = idx % (C / 4);
    const size_t r = idx / (C / 4);
    const int crop = r / hw;
    const float4 v = *reinterpret_cast<const float4*>(p + r * C + c4 * 4);
    float4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c4 * 4 + k;
        const float y = bn_y((f4get(v, k) - mean[c]) * invstd[c], g[c], be[c]);
        const bool kept = c < creal && keep[(size_t)crop * creal + c] != 0;
        f4set(o, k, kept ? fmaxf(y, 0.f) * scale : 0.f);
    }
    *reinterpret_cast<float4*>(a + r * C + c4 * 4) = o;
}

// v110: sums of dy and dy * x-hat per channel over the pooled rows, dy = da keep scale [y > 0]: partial[block][2][C] (k_t_bn_stats's walk)
template <int C>
__global__ __launch_bounds__(256) void k_tarch_bn_bwd_stats(const float* __restrict__ da, const float* __restrict__ p, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ g, const float* __restrict__ be,
                                                            const uint8_t* __restrict__ keep, const int creal, const float scale, const size_t rows, const int hw,
                                                            double* __restrict__ partial) {
    constexpr int LC = C / 4, RL = 256 / LC;
    __shared__ double sh[RL * C];
    const int tid = threadIdx.x, cl = tid % LC, rl = tid / LC;
    float mn[4], iv[4], ga[4], bt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int c = cl * 4 + k; mn[k] = mean[c]; iv[k] = invstd[c]; ga[k] = g[c]; bt[k] = be[c]; }
    double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (size_t r = (size_t)blockIdx.x * RL + rl; r < rows; r += (size_t)gridDim.x * RL) {
        const int crop = r / hw;
        const float4 v = *reinterpret_cast<const float4*>(p + r * C + cl * 4);
        const float4 d = *reinterpret_cast<const float4*>(da + r * C + cl * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = cl * 4 + k;
            const float xh = (f4get(v, k) - mn[k]) * iv[k];
            const bool open = c < creal && keep[(size_t)crop * creal + c] != 0 && bn_y(xh, ga[k], bt[k]) > 0.f;
            const float dy = open ? f4get(d, k) * scale : 0.f;
            acc[0][k] += dy; acc[1][k] += (double)dy * xh;
        }
    }
    block_columns<C, 2>(acc, sh, partial);
}

// ------------------------------------------------------------------------------------------------
// the way back through the pool: dz written over z [n][H][W][C] for every pixel -- dp at the window's stored arg-max, 0 at the other three, 0 in
// the odd last row / column that no window holds (the walk is over ceil(H/2) x ceil(W/2) windows, masked).  v110: dp = gamma invstd (dy - mean(dy) -
// x-hat mean(dy x-hat)), the means over the n (H/2)(W/2) pooled elements; V100: dp = da scale where the byte is not 4.  The column sums of what was
// written are the convolution bias's gradient: partial[block][1][C].  A thread's elements lie a grid-stride apart (a multiple of C / 4)
// ------------------------------------------------------------------------------------------------
template <int C, bool V100>
__global__ __launch_bounds__(256) void k_tarch_unpool(const float* __restrict__ da, const float* __restrict__ p, const uint32_t* __restrict__ arg4,
                                                      float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                      const float* __restrict__ g, const float* __restrict__ be, const uint8_t* __restrict__ keep, const int creal,
                                                      const float scale, const float* __restrict__ sums, const float inv_count, const int n, const int H, const int W,
                                                      double* __restrict__ partial) {
    constexpr int LC = C / 4, RL = 256 / LC;
    __shared__ double sh[RL * C];
    const int Hp = H / 2, Wp = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const size_t total = (size_t)n * Hc * Wc * LC;
    const int c4 = threadIdx.x % LC;
    float mn[4], iv[4], ga[4], bt[4], m1[4], m2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c4 * 4 + k;
        mn[k] = iv[k] = ga[k] = bt[k] = m1[k] = m2[k] = 0.f;
        if (!V100) { mn[k] = mean[c]; iv[k] = invstd[c]; ga[k] = g[c]; bt[k] = be[c]; m1[k] = sums[c] * inv_count; m2[k] = sums[C + c] * inv_count; }
    }
    double acc[1][4] = {{0, 0, 0, 0}};
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t pos = idx / LC;
        const int px = pos % Wc, py = (pos / Wc) % Hc, crop = pos / ((size_t)Hc * Wc);
        const bool pooled = py < Hp && px < Wp;                         // all four pixels exist and the pool has an output here
        const bool vq[4] = {true, 2 * px + 1 < W, 2 * py + 1 < H, 2 * px + 1 < W && 2 * py + 1 < H};
        float4 o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pooled) {
            const size_t r = ((size_t)crop * Hp + py) * Wp + px;
            const float4 d = *reinterpret_cast<const float4*>(da + r * C + c4 * 4);
            const uint32_t packed = arg4[r * LC + c4];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!V100) v = *reinterpret_cast<const float4*>(p + r * C + c4 * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c4 * 4 + k;
                const uint32_t arg = (packed >> (8 * k)) & 0xffu;
                float dp = 0.f;
                if (V100) {
                    dp = arg < 4 ? f4get(d, k) * scale : 0.f;
                } else if (c < creal) {
                    const float xh = (f4get(v, k) - mn[k]) * iv[k];
                    const bool open = keep[(size_t)crop * creal + c] != 0 && bn_y(xh, ga[k], bt[k]) > 0.f;
                    const float dy = open ? f4get(d, k) * scale : 0.f;
                    dp = ga[k] * iv[k] * (dy - m1[k] - xh * m2[k]);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) f4set(o[q], k, arg == (uint32_t)q ? dp : 0.f);
                if (arg < 4) acc[0][k] += dp;
            }
        }
        float* base = z + (((size_t)crop * H + 2 * py) * W + 2 * px) * C + c4 * 4;
        const size_t qoff[4] = {0, (size_t)C, (size_t)W * C, (size_t)W * C + C};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (vq[q]) *reinterpret_cast<float4*>(base + qoff[q]) = o[q];
    }
    block_columns<C, 1>(acc, sh, partial);
}

// ------------------------------------------------------------------------------------------------
// the heads.  hsum [n][100] is fc1's output without its bias (k_tany_fc1_sum)
// ------------------------------------------------------------------------------------------------
// v110: BatchNorm1d's batch statistics of h = hsum + b1: one thread per column, the n rows in ascending order (eight loads in flight), in double;
// mean, invstd from the biased variance, the running statistics from the unbiased one (left alone when the step was refused)
__global__ __launch_bounds__(128) void k_tarch_bn1d_stats(const float* __restrict__ hsum, const float* __restrict__ b1, const int n, const float momentum,
                                                          float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ run_mean,
                                                          float* __restrict__ run_var, const int32_t* __restrict__ refused) {
    const int j = threadIdx.x;
    if (j >= HID) return;
    const float b = b1[j];
    double s1 = 0, s2 = 0;
    for (int s0 = 0; s0 < n; s0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = s0 + k < n ? hsum[(size_t)(s0 + k) * HID + j] + b : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) if (s0 + k < n) { s1 += v[k]; s2 += (double)v[k] * v[k]; }
    }
    const double m = s1 / n;
    double var = s2 / n - m * m;
    if (var < 0) var = 0;
    mean[j] = (float)m;
    invstd[j] = (float)(1.0 / sqrt(var + (double)EPS_BN));
    if (*refused) return;
    const double unbiased = n > 1 ? var * n / (n - 1) : var;
    run_mean[j] = (1.f - momentum) * run_mean[j] + momentum * (float)m;
    run_var[j] = (1.f - momentum) * run_var[j] + momentum * (float)unbiased;
}

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

// one block per sample: fc1 bias (+ BatchNorm1d with the given mean / invstd: the batch's or the running ones) + ReLU + dropout + fc2 + softmax cross
// entropy, and the way back to the gradient at the ReLU's input: gy [n][100] (v100: that is d(fc1 output); v110: d(BatchNorm output)).  k_t_head's
// expressions for the logits, the loss, the arg-max and the softmax.  probs != null: a prediction -- the softmax rows and nothing else
template <bool BN>
__global__ __launch_bounds__(128) void k_tarch_head(const float* __restrict__ hsum, const int n, const float* __restrict__ b1, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, const float* __restrict__ g, const float* __restrict__ be,
                                                    const uint8_t* __restrict__ keep /*[n][100]*/, const float scale, const float* __restrict__ w2 /*[C][100]*/,
                                                    const float* __restrict__ b2, const int32_t* __restrict__ targets, const int classes,
                                                    float* __restrict__ xhat /*[n][100]*/, float* __restrict__ hd /*[n][100]*/, float* __restrict__ dl /*[n][C]*/,
                                                    float* __restrict__ gy_out /*[n][100]*/, float* __restrict__ loss, int32_t* __restrict__ correct,
                                                    float* __restrict__ probs) {
    __shared__ float red[128];
    __shared__ float s_d[HID];
    __shared__ float s_dl[1024];
    __shared__ int s_arg[128];
    const int tid = threadIdx.x, s = blockIdx.x;
    const bool act = tid < HID;
    float xh = 0.f, y = 0.f;
    bool kp = false;
    if (act) {
        const float h = hsum[(size_t)s * HID + tid] + b1[tid];
        if (BN) { xh = (h - mean[tid]) * invstd[tid]; y = bn_y(xh, g[tid], be[tid]); }
        else y = h;
        kp = keep[(size_t)s * HID + tid] != 0;
        const float d = kp ? fmaxf(y, 0.f) * scale : 0.f;
        s_d[tid] = d;
        if (!probs) { hd[(size_t)s * HID + tid] = d; if (BN) xhat[(size_t)s * HID + tid] = xh; }
    }
    __syncthreads();
    float lmax = -INFINITY;
    int larg = 0x7fffffff;
    for (int c = tid; c < classes; c += 128) {
        float acc = b2[c];
        const float* wr = w2 + (size_t)c * HID;
        for (int j = 0; j < HID; ++j) acc += s_d[j] * wr[j];
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
    float se = 0.f;
    for (int c = tid; c < classes; c += 128) se += expf(s_dl[c] - gmax);
    const float sum = block_sum128(se, red);
    const float lse = gmax + logf(sum);
    if (probs) {                                               // (uniform)
        for (int c = tid; c < classes; c += 128) probs[(size_t)s * classes + c] = expf(s_dl[c] - lse);
        return;
    }
    int target = targets[s];
    if (target < 0 || target >= classes) target = 0;       // (memory safety only: k_t_check_targets has already refused this step)
    if (tid == 0) {
        loss[s] = lse - s_dl[target];
        correct[s] = s_arg[0] == target ? 1 : 0;
    }
    __syncthreads();
    const float invn = 1.0f / (float)n;
    for (int c = tid; c < classes; c += 128) {
        const float pr = expf(s_dl[c] - lse);
        const float gl = (pr - (c == target ? 1.f : 0.f)) * invn;
        s_dl[c] = gl;
        dl[(size_t)s * classes + c] = gl;
    }
    __syncthreads();
    if (act) {
        float dd = 0.f;
        for (int c = 0; c < classes; ++c) dd += s_dl[c] * w2[(size_t)c * HID + tid];
        gy_out[(size_t)s * HID + tid] = (kp && y > 0.f) ? dd * scale : 0.f;      // through dropout and the ReLU gate
    }
}

// v110: sums[0][j] = sum_n dy = d beta, sums[1][j] = sum_n dy x-hat = d gamma: one thread per column, the rows in ascending order, in double
__global__ __launch_bounds__(128) void k_tarch_bn1d_sums(const float* __restrict__ dy, const float* __restrict__ xhat, const int n, float* __restrict__ sums /*[2][100]*/,
                                                         float* __restrict__ d_gamma, float* __restrict__ d_beta) {
    const int j = threadIdx.x;
    if (j >= HID) return;
    double s1 = 0, s2 = 0;
    for (int s0 = 0; s0 < n; s0 += 8) {
        float a[8], b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const bool ok = s0 + k < n; a[k] = ok ? dy[(size_t)(s0 + k) * HID + j] : 0.f; b[k] = ok ? xhat[(size_t)(s0 + k) * HID + j] : 0.f; }
#pragma unroll
        for (int k = 0; k < 8; ++k) if (s0 + k < n) { s1 += a[k]; s2 += (double)a[k] * b[k]; }
    }
    sums[j] = (float)s1; sums[HID + j] = (float)s2;
    d_beta[j] = (float)s1; d_gamma[j] = (float)s2;
}

// v110: dh = gamma invstd (dy - mean(dy) - x-hat mean(dy x-hat)) over the batch
__global__ __launch_bounds__(256) void k_tarch_bn1d_dh(const float* __restrict__ dy, const float* __restrict__ xhat, const float* __restrict__ sums,
                                                       const float* __restrict__ g, const float* __restrict__ invstd, const int n, float* __restrict__ dh) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * HID) return;
    const int j = idx % HID;
    const float inv_n = 1.0f / (float)n;
    dh[idx] = g[j] * invstd[j] * (dy[idx] - sums[j] * inv_n - xhat[idx] * (sums[HID + j] * inv_n));
}

// parameter gradients of the head: fc2 weight / bias and fc1 bias = sum_n dh (v110: rounding noise around 0, the bias feeds a BatchNorm); one thread
// per element, the samples in order, eight operands in flight
__global__ __launch_bounds__(256) void k_tarch_head_grads(const float* __restrict__ dl, const float* __restrict__ hd, const float* __restrict__ dh, const int n,
                                                          const int classes, float* __restrict__ g_w2, float* __restrict__ g_b2, float* __restrict__ g_b1) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nw = classes * HID;
    if (idx >= nw + classes + HID) return;
    const float* pa; const float* pb = nullptr; size_t sa, sb = 0; float* dst;
    if (idx < nw) { const int c = idx / HID, j = idx % HID; pa = dl + c; sa = classes; pb = hd + j; sb = HID; dst = g_w2 + idx; }
    else if (idx < nw + classes) { pa = dl + (idx - nw); sa = classes; dst = g_b2 + (idx - nw); }
    else { pa = dh + (idx - nw - classes); sa = HID; dst = g_b1 + (idx - nw - classes); }
    float acc = 0.f;
    for (int s0 = 0; s0 < n; s0 += 8) {
        float va[8], vb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const int s = s0 + k < n ? s0 + k : n - 1; va[k] = pa[(size_t)s * sa]; vb[k] = pb ? pb[(size_t)s * sb] : 1.f; }
#pragma unroll
        for (int k = 0; k < 8; ++k) if (s0 + k < n) acc += va[k] * vb[k];
    }
    *dst = acc;
}

// ------------------------------------------------------------------------------------------------
// host side: one trainer for the three networks of the one-stream chain.  A network is data (Net, and its tensors: train_tensors.h) plus the two
// functions of its block kind and its head, chosen once in chain_trainer_create; the walk below is the same for all of them
// ------------------------------------------------------------------------------------------------
struct Block {
    int C, CI, creal, h, w;                 // z [n][h][w][C]; pl, arg, a, da [n][h/2][w/2][C]
    int slot;                               // its first tensor slot
    float *z = nullptr, *pl = nullptr, *a = nullptr, *da = nullptr;
    uint32_t* arg = nullptr;
    float* wb = nullptr;                    // flipped + transposed weights of its data gradient (blocks 2, 3)
    int cic = 0, dg_co = 0, dg_cic = 0;     // its weight image: the parameter layout's chunk, the data gradient's tile and chunk
};

struct ChainTrainer;
struct Net {
    TrainNet tensors;                       // its row of train_tensors.h: taps, slots, state_dict order, mask planes, Adam's buffers
    float drop[4];                          // the network's own dropout rates (trexhip_train_params.dropout is V118_3's)
    bool arg, pl, bn_head;                  // a block keeps the pool's arg-max bytes (v100, v110) and the raw pooled plane (v110); BatchNorm1d behind fc1
    // z -> a of one block.  train: batch statistics + the dropout masks; eval: running statistics, the caller's masks keep everything
    void (*block_forward)(ChainTrainer*, hipStream_t, const Block&, int n, const uint8_t* kp, float scale, bool train);
    // da -> dz written over z, the gradients of gamma and beta where it has them; returns the workgroups whose column sums red_bias holds
    int (*block_backward)(ChainTrainer*, hipStream_t, const Block&, int n, const uint8_t* kp, float scale);
    void (*head)(ChainTrainer*, hipStream_t, int n, const uint8_t* kp, float scale, const int32_t* targets, bool train, float* probs);
};

struct ChainTrainer : TrainerCore {
    const Net* net = nullptr;
    TrainAnyGeom geom{};
    Block L[3];
    float *part = nullptr, *part1 = nullptr, *stat = nullptr /*4 x (mean, invstd, sums[2]) x 128*/;
    float *hpart = nullptr, *hsum = nullptr, *xhat = nullptr, *hd = nullptr, *dl = nullptr, *dy = nullptr, *dh = nullptr;
    double *red = nullptr, *red_bias = nullptr;
    float scale(int i, bool train) const { return train ? 1.0f / (1.0f - net->drop[i]) : 1.f; }
    const uint8_t* plane(const uint8_t* keep, int n, int i) const { return keep + (size_t)n * tt.keep_off[i]; }

    int refuse_step(const char* who, int n) override {
        // BatchNorm over one value per channel: the reference raises "Expected more than 1 value per channel when training"
        if (!net->bn_head || n >= 2) return TREXHIP_OK;
        set_error(std::string(who) + ": a v110 training step needs n >= 2 (BatchNorm1d over the batch: more than 1 value per channel)");
        return TREXHIP_E_INVALID;
    }
    const uint8_t* begin_step(hipStream_t s, int n, const uint8_t* injected) override;
    void forward(hipStream_t s, const float* x, const int32_t* targets, int n, const uint8_t* keep, bool train, float* probs) override;
    void backward(hipStream_t s, const float* x, int n, const uint8_t* keep) override;
    size_t blob_bytes() const override { return version == TREXHIP_NET_CATEGORY ? category_blob_bytes(classes, CH, W, H) : arch_blob_bytes(version, classes, CH, W, H); }
    void write_blob_header(void* blob) const override {
        if (version == TREXHIP_NET_CATEGORY) { write_category_blob_header(blob, classes, W, H, CH); return; }
        write_weight_blob_header(blob, classes, W, H, CH);
        static_cast<int32_t*>(blob)[6] = version;
    }
};

template <bool V100>
void launch_pool(hipStream_t s, const Block& L, const uint8_t* keep, float scale, float* out, int n) {
    const size_t total = (size_t)n * (L.h / 2) * (L.w / 2) * (L.C / 4);
    if (!total) return;
    const auto fn = L.C == 16 ? &k_tarch_pool<16, V100> : L.C == 64 ? &k_tarch_pool<64, V100> : &k_tarch_pool<128, V100>;
    hipLaunchKernelGGL(fn, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, L.z, keep, L.creal, scale, out, L.arg, n, L.h, L.w);
}

// mean and invstd of block i for its BatchNorm over `rows` rows of d: the batch's (and the running statistics move) or the running ones
void block_stats(ChainTrainer* t, hipStream_t s, const Block& L, const float* d, size_t rows, bool train) {
    float* mean = t->stat + L.slot / 6 * 512;
    if (train) {
        t_bn_stats(s, L.C, d, rows, t->red);
        t_fin_bn_stats(s, t->red, T_RED_BLOCKS, L.C, (double)rows, t->p.bn_momentum, mean, mean + 128, t->param(L.slot + K_RM), t->param(L.slot + K_RV), t->bad_target);
    } else {
        t_bn_from_running(s, t->param(L.slot + K_RM), t->param(L.slot + K_RV), L.C, mean, mean + 128);
    }
}

// ---- pool only (v100)
void pool_forward(ChainTrainer*, hipStream_t s, const Block& L, int n, const uint8_t* kp, float scale, bool) { launch_pool<true>(s, L, kp, scale, L.a, n); }

// the grid of k_tarch_unpool -- whole rounds: every workgroup takes the same number of elements
size_t unpool_blocks(const Block& L, int n) {
    const size_t total = (size_t)n * ((L.h + 1) / 2) * ((L.w + 1) / 2) * (L.C / 4);
    const size_t nb0 = (total + 255) / 256, per = (nb0 + T_BWD_BLOCKS - 1) / T_BWD_BLOCKS;
    return (nb0 + per - 1) / per;
}

// ---- pool, then BatchNorm over the pooled rows (v110)
void pool_bn_forward(ChainTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* kp, float scale, bool train) {
    launch_pool<false>(s, L, nullptr, 1.f, L.pl, n);
    float* mean = t->stat + L.slot / 6 * 512;
    const int hw = (L.h / 2) * (L.w / 2);
    const size_t rows = (size_t)n * hw;
    block_stats(t, s, L, L.pl, rows, train);
    const size_t lanes = rows * (L.C / 4);
    const auto fn = L.C == 16 ? &k_tarch_bn_apply<16> : L.C == 64 ? &k_tarch_bn_apply<64> : &k_tarch_bn_apply<128>;
    hipLaunchKernelGGL(fn, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, L.pl, mean, mean + 128, t->param(L.slot + K_G), t->param(L.slot + K_BE), kp, L.creal, scale,
                       L.a, rows, hw);
}

int pool_bn_backward(ChainTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* kp, float scale) {
    float* mean = t->stat + L.slot / 6 * 512;
    float* invstd = mean + 128;
    float* sums = mean + 256;
    const int hw = (L.h / 2) * (L.w / 2);
    const size_t rows = (size_t)n * hw;
    const float *g = t->param(L.slot + K_G), *be = t->param(L.slot + K_BE);
    {
        const auto fn = L.C == 16 ? &k_tarch_bn_bwd_stats<16> : L.C == 64 ? &k_tarch_bn_bwd_stats<64> : &k_tarch_bn_bwd_stats<128>;
        hipLaunchKernelGGL(fn, dim3(T_RED_BLOCKS), dim3(256), 0, s, L.da, L.pl, mean, invstd, g, be, kp, L.creal, scale, rows, hw, t->red);
    }
    t_fin_bn_bwd(s, t->red, T_RED_BLOCKS, L.C, sums, t->grad(L.slot + K_G), t->grad(L.slot + K_BE));
    const size_t nb = unpool_blocks(L, n);
    const float inv_count = (float)(1.0 / (double)std::max<size_t>(rows, 1));
    const auto fn = L.C == 16 ? &k_tarch_unpool<16, false> : L.C == 64 ? &k_tarch_unpool<64, false> : &k_tarch_unpool<128, false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(256), 0, s, L.da, L.pl, L.arg, L.z, mean, invstd, g, be, kp, L.creal, scale, sums, inv_count, n, L.h, L.w, t->red_bias);
    return (int)nb;
}

// (v100's way back stands behind v110's so that the kernel instances keep the order the compiler has always emitted them in; the heads likewise)
int pool_backward(ChainTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* kp, float scale) {
    const size_t nb = unpool_blocks(L, n);
    const auto fn = L.C == 16 ? &k_tarch_unpool<16, true> : L.C == 64 ? &k_tarch_unpool<64, true> : &k_tarch_unpool<128, true>;
    hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(256), 0, s, L.da, nullptr, L.arg, L.z, nullptr, nullptr, nullptr, nullptr, kp, L.creal, scale, nullptr, 0.f, n, L.h, L.w,
                       t->red_bias);
    return (int)nb;
}

// ---- BatchNorm over all n h w pixels of the convolution's plane, then the pool with element-wise masks (the category network): train_any.hip's
// block kernels with `creal`
void bn_pool_forward(ChainTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* kp, float scale, bool train) {
    float* mean = t->stat + L.slot / 6 * 512;
    block_stats(t, s, L, L.z, (size_t)n * L.h * L.w, train);
    tany_bn_pool(s, L.C, L.z, mean, mean + 128, t->param(L.slot + K_G), t->param(L.slot + K_BE), kp, scale, L.a, n, L.h, L.w, L.creal);
}

int bn_pool_backward(ChainTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* kp, float scale) {
    float* mean = t->stat + L.slot / 6 * 512;
    float* invstd = mean + 128;
    float* sums = mean + 256;
    const float *g = t->param(L.slot + K_G), *be = t->param(L.slot + K_BE);
    tany_pool_bwd_stats(s, L.C, T_RED_BLOCKS, L.da, L.z, mean, invstd, g, be, kp, scale, n, L.h, L.w, t->red, L.creal);
    t_fin_bn_bwd(s, t->red, T_RED_BLOCKS, L.C, sums, t->grad(L.slot + K_G), t->grad(L.slot + K_BE));
    const float inv_count = (float)(1.0 / ((double)n * L.h * L.w));      // the means run over every pixel of the plane
    return tany_bn_bwd(s, L.C, T_BWD_BLOCKS, L.da, L.z, mean, invstd, g, be, kp, scale, sums, inv_count, n, L.h, L.w, t->red_bias, L.creal);
}

// ---- the heads: hsum -> loss, arg-max and the gradient at the ReLU's input (dh; v110: dy, in front of its BatchNorm1d's way back)
void head_bn(ChainTrainer* t, hipStream_t s, int n, const uint8_t* kp, float scale, const int32_t* targets, bool train, float* probs) {
    float* mean = t->stat + 3 * 512;
    float* invstd = mean + 128;
    if (train) hipLaunchKernelGGL(k_tarch_bn1d_stats, dim3(1), dim3(128), 0, s, t->hsum, t->param(S_F1B), n, t->p.bn_momentum, mean, invstd, t->param(S_RM4), t->param(S_RV4), t->bad_target);
    else t_bn_from_running(s, t->param(S_RM4), t->param(S_RV4), HID, mean, invstd);
    hipLaunchKernelGGL(k_tarch_head<true>, dim3(n), dim3(128), 0, s, t->hsum, n, t->param(S_F1B), mean, invstd, t->param(S_G4), t->param(S_BE4), kp, scale, t->param(S_F2W),
                       t->param(S_F2B), targets, t->classes, t->xhat, t->hd, t->dl, t->dy, t->loss, t->correct, probs);
}

void head_plain(ChainTrainer* t, hipStream_t s, int n, const uint8_t* kp, float scale, const int32_t* targets, bool, float* probs) {
    hipLaunchKernelGGL(k_tarch_head<false>, dim3(n), dim3(128), 0, s, t->hsum, n, t->param(S_F1B), nullptr, nullptr, nullptr, nullptr, kp, scale, t->param(S_F2W), t->param(S_F2B),
                       targets, t->classes, nullptr, t->hd, t->dl, t->dh, t->loss, t->correct, probs);
}

//                    tensors         dropout rates                 arg    pl     BN head  z -> a           da -> dz          head
const Net NET_V100 = {TRAIN_V100,     {0.25f, 0.25f, 0.25f, 0.5f},  true,  false, false,   pool_forward,    pool_backward,    head_plain};
const Net NET_V110 = {TRAIN_V110,     {0.25f, 0.25f, 0.25f, 0.25f}, true,  true,  true,    pool_bn_forward, pool_bn_backward, head_bn};
const Net NET_CAT  = {TRAIN_CATEGORY, {0.25f, 0.25f, 0.25f, 0.25f}, false, false, false,   bn_pool_forward, bn_pool_backward, head_plain};

// the three planes behind the blocks share a rate and are one draw; the head's plane comes from another stream of the same counter hash
const uint8_t* ChainTrainer::begin_step(hipStream_t s, int n, const uint8_t* injected) {
    if (injected) return injected;
    t_masks(s, keep, (size_t)n * tt.keep_off[3], p.seed, (uint64_t)step, net->drop[0]);
    t_masks(s, keep + (size_t)n * tt.keep_off[3], (size_t)n * HID, p.seed ^ 0xD1B54A32D192ED03ull, (uint64_t)step, net->drop[3]);
    return keep;
}

void ChainTrainer::forward(hipStream_t s, const float* x, const int32_t* targets, int n, const uint8_t* keep, bool train, float* probs) {
    tany_conv1(s, geom, n, x, param(K_W), param(K_B), L[0].z);
    net->block_forward(this, s, L[0], n, plane(keep, n, 0), scale(0, train), train);
    for (int i = 1; i < 3; ++i) {
        tany_conv_fwd(s, geom, i, n, L[i - 1].a, param(L[i].slot + K_W), param(L[i].slot + K_B), L[i].z);
        net->block_forward(this, s, L[i], n, plane(keep, n, i), scale(i, train), train);
    }
    tany_fc1(s, geom, n, L[2].a, param(S_F1W), hpart, hsum);
    net->head(this, s, n, plane(keep, n, 3), scale(3, train), targets, train, probs);
}

void ChainTrainer::backward(hipStream_t s, const float* x, int n, const uint8_t* keep) {
    if (net->bn_head) {
        float* mean = stat + 3 * 512;
        hipLaunchKernelGGL(k_tarch_bn1d_sums, dim3(1), dim3(128), 0, s, dy, xhat, n, mean + 256, grad(S_G4), grad(S_BE4));
        hipLaunchKernelGGL(k_tarch_bn1d_dh, dim3((n * HID + 255) / 256), dim3(256), 0, s, dy, xhat, mean + 256, param(S_G4), mean + 128, n, dh);
    }
    hipLaunchKernelGGL(k_tarch_head_grads, dim3((classes * HID + classes + HID + 255) / 256), dim3(256), 0, s, dl, hd, dh, n, classes, grad(S_F2W), grad(S_F2B), grad(S_F1B));
    tany_fc1_wgrad(s, geom, n, L[2].a, dh, grad(S_F1W));
    t_loss(s, loss, correct, n, out2);
    tany_fc1_dgrad(s, geom, n, dh, param(S_F1W), L[2].da);
    for (int i = 2; i >= 0; --i) {
        const Block& B = L[i];
        const int nb = net->block_backward(this, s, B, n, plane(keep, n, i), scale(i, true));
        t_fin_bias(s, red_bias, nb, B.C, grad(B.slot + K_B));
        if (i == 0) break;
        // the weight gradient and the data gradient of blocks 2 and 3
        tany_wgrad(s, geom, i, n, L[i - 1].a, B.z, part);
        t_wgrad_reduce(s, part, geom.wg_shares(i, n), B.CI, B.C, B.cic, grad(B.slot + K_W), geom.taps);
        t_repack_bwd(s, param(B.slot + K_W), B.CI, B.C, B.cic, B.dg_co, B.dg_cic, B.wb, geom.taps);
        tany_conv_dgrad(s, geom, i, n, B.z, B.wb, L[i - 1].da);
    }
    tany_wgrad1(s, geom, n, x, L[0].z, part1);
    t_reduce(s, part1, n * geom.wg1_tiles, CH * geom.taps * geom.taps * 16, grad(K_W));
}

}  // namespace

// blob: a category blob ('TRXC', the parser of trexhip_categorize_load_weights: its codes and field names) or an identity blob whose header names
// v100 or v110 (the parser of trexhip_load_weights)
int chain_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, TrainerCore** out) {
    const char* who = "trexhip_trainer_create";
    if (const int rc = check_train_params(p)) return rc;
    ArchBlob ab;
    const bool cat = blob_is_category(blob, bytes);
    if (const int rc = cat ? parse_category_blob(blob, bytes, who, &ab) : parse_arch_blob(blob, bytes, who, &ab)) return rc;
    if (hipSetDevice(ctx->p.device) != hipSuccess) { set_error("trexhip_trainer_create: hipSetDevice failed"); return TREXHIP_E_DEVICE; }
    ChainTrainer* t = new ChainTrainer();
    t->net = cat ? &NET_CAT : ab.id == TREXHIP_NET_V110 ? &NET_V110 : &NET_V100;
    t->ctx = ctx; t->version = cat ? TREXHIP_NET_CATEGORY : ab.id; t->classes = ab.classes; t->CH = ab.CH; t->max_n = p->max_batch; t->p = *p;
    t->W = ab.W; t->H = ab.H;
    t->tt = train_tensors(t->net->tensors, ab.W, ab.H, ab.CH, ab.classes);
    t->geom = train_any_geom(ab.W, ab.H, ab.CH, t->tt.taps);
    const float* src[S_COUNT] = {};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 6; ++k) src[6 * i + k] = ab.conv[i][k];
    src[S_F1W] = ab.fc1w; src[S_F1B] = ab.fc1b; src[S_F2W] = ab.fc2w; src[S_F2B] = ab.fc2b;
    for (int k = 0; k < 4; ++k) src[S_G4 + k] = ab.bn1d[k];
    Block* L = t->L;
    for (int i = 0; i < 3; ++i) { L[i].C = t->geom.L[i].C; L[i].CI = t->geom.L[i].CI; L[i].creal = i == 2 ? t->tt.c3 : L[i].C; L[i].h = t->geom.L[i].h; L[i].w = t->geom.L[i].w; L[i].slot = 6 * i; }
    L[1].cic = 16; L[1].dg_cic = 16; L[1].dg_co = 32;            // conv2's data gradient: 16 real channels in a 32-wide tile
    L[2].cic = 32; L[2].dg_cic = 32; L[2].dg_co = 64;
    // ---- memory
    const size_t n = (size_t)t->max_n, T2 = (size_t)t->tt.taps * t->tt.taps;
    int rc = TREXHIP_OK;
#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)
    for (int i = 0; i < 3; ++i) {
        const size_t pooled = t->geom.a_floats(i, n);
        TRY(t->mem.device(&L[i].z, t->geom.z_floats(i, n), who)); TRY(t->mem.device(&L[i].a, pooled, who)); TRY(t->mem.device(&L[i].da, pooled, who));
        if (t->net->arg) TRY(t->mem.device(&L[i].arg, pooled / 4, who));
        if (t->net->pl) TRY(t->mem.device(&L[i].pl, pooled, who));
    }
    TRY(t->mem.device(&L[2].wb, 4 * T2 * 32 * 64, who)); TRY(t->mem.device(&L[1].wb, 2 * T2 * 32 * 32, who));
    TRY(t->mem.device(&t->part, t->geom.part_floats(), who)); TRY(t->mem.device(&t->part1, t->geom.part1_floats(n), who));
    TRY(t->mem.device(&t->red_bias, (size_t)T_BWD_BLOCKS * 128, who)); TRY(t->mem.device(&t->red, (size_t)T_BWD_BLOCKS * 2 * 128, who));
    TRY(t->mem.device(&t->stat, (size_t)4 * 512, who));
    TRY(t->mem.device(&t->hpart, t->geom.hpart_floats(n), who)); TRY(t->mem.device(&t->hsum, n * HID, who));
    TRY(t->mem.device(&t->hd, n * HID, who)); TRY(t->mem.device(&t->dl, n * ab.classes, who)); TRY(t->mem.device(&t->dh, n * HID, who));
    if (t->net->bn_head) { TRY(t->mem.device(&t->xhat, n * HID, who)); TRY(t->mem.device(&t->dy, n * HID, who)); }
    TRY(tany_attrs());
    TRY(t->init_state(src, who));
#undef TRY
    if (rc != TREXHIP_OK) { delete t; return rc; }
    *out = t;
    return TREXHIP_OK;
}

}  // namespace trexhip
