// train_arch.hip -- the training step of the identity networks v100 and v110 (visual_identification_network_torch.py:262-382, train mode;
// the loop body visual_recognition_torch.py:1137-1158) at every size they load: W, H = 8..256, CH = 1 or 3, NHWC fp32, exact fp32 arithmetic at
// both values of trexhip_train_params.precision.
//
//   v100   [conv5x5 'same' -> ReLU -> MaxPool2 -> Dropout2d(0.25)] x3 -> flatten (NCHW) -> fc1 -> ReLU -> Dropout(0.5) -> fc2 -> cross entropy
//   v110   [conv5x5 'same' -> MaxPool2 -> BatchNorm2d -> ReLU -> Dropout2d(0.25)] x3 -> flatten -> fc1 -> BatchNorm1d -> ReLU -> Dropout(0.25) -> fc2
//
// The convolutions are V118_3's with conv3 at 100 outputs instead of 128, so the three roles of every convolution, both conv1 kernels and fc1 are
// train_any.hip's (tany_*), and the reductions, Adam, the masks, the target check and the loss sum train.hip's (train_shared.h).  The 100 channels
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
#include "train_shared.h"
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
constexpr int CP[3] = {16, 64, 128};                     // channels of a block as the kernels see them
constexpr int CR[3] = {16, 64, 100};                     // ... and as torch does
// keep masks of one step: four planes back to back, [n][16] [n][64] [n][100] [n][100]; plane i starts at keep + n * KEEP_OFF[i]
constexpr int KEEP_OFF[4] = {0, 16, 16 + 64, 16 + 64 + 100}, KEEP_ROW = 16 + 64 + 100 + HID;
// the architecture's dropout rates (trexhip_train_params.dropout is V118_3's)
constexpr float P_DROP[2][4] = {{0.25f, 0.25f, 0.25f, 0.5f}, {0.25f, 0.25f, 0.25f, 0.25f}};

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
// host side
// ------------------------------------------------------------------------------------------------
// the tensors as the trainer holds them: six slots per block (weight, bias, gamma, beta, running mean, running variance), then the head's
enum { S_F1W = 18, S_F1B, S_G4, S_BE4, S_RM4, S_RV4, S_F2W, S_F2B, S_COUNT };
enum { K_W, K_B, K_G, K_BE, K_RM, K_RV };

struct Block {
    int C, CI, creal, h, w;                 // z [n][h][w][C]; pl, arg, a, da [n][h/2][w/2][C]
    int slot;                               // its first tensor slot
    float *z = nullptr, *pl = nullptr, *a = nullptr, *da = nullptr;
    uint32_t* arg = nullptr;
    float* wb = nullptr;                    // flipped + transposed weights of its data gradient (blocks 2, 3)
    int cic = 0, dg_co = 0, dg_cic = 0;     // its weight image: the parameter layout's chunk, the data gradient's tile and chunk
};

}  // namespace

struct ArchTrainer {
    trexhip_ctx* ctx = nullptr;
    int version = 0, classes = 0, CH = 1, max_n = 0, W = 0, H = 0;
    bool bn = false;                        // v110
    TrainAnyGeom geom{};
    trexhip_train_params p{};
    int64_t step = 0;
    int n_tensors = 0, order[S_COUNT] = {};           // the version's state_dict order -> slots
    size_t off[S_COUNT + 1] = {}, cnt[S_COUNT] = {}, isz[S_COUNT] = {};      // offset, torch's element count, elements held (padded)
    size_t total = 0;
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr;
    Block L[3];
    float *part = nullptr, *part1 = nullptr, *stat = nullptr /*4 x (mean, invstd, sums[2]) x 128*/;
    float *hpart = nullptr, *hsum = nullptr, *xhat = nullptr, *hd = nullptr, *dl = nullptr, *dy = nullptr, *dh = nullptr, *loss = nullptr, *out2 = nullptr;
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
        case 0: { const size_t tap = i % 25, c = (i / 25) % CH, co = i / (25 * (size_t)CH); return (c * 25 + tap) * 16 + co; }
        case 6: { const size_t tap = i % 25, ci = (i / 25) % 16, co = i / 400; return (tap * 16 + ci) * 64 + co; }
        case 12: { const size_t tap = i % 25, ci = (i / 25) % 64, co = i / 1600; return (((ci / 32) * 25 + tap) * 32 + ci % 32) * 128 + co; }
        case S_F1W: { const size_t K = 100 * P, k = i % K, o = i / K, c = k / P, hw = k % P; return (hw * 128 + c) * HID + o; }
        default: return i;
    }
}

void trainer_free(ArchTrainer* t) {
    if (!t) return;
    t->mem.free_all();
    delete t;
}

template <bool V100>
void launch_pool(hipStream_t s, const Block& L, const uint8_t* keep, float scale, float* out, int n) {
    const size_t total = (size_t)n * (L.h / 2) * (L.w / 2) * (L.C / 4);
    if (!total) return;
    const auto fn = L.C == 16 ? &k_tarch_pool<16, V100> : L.C == 64 ? &k_tarch_pool<64, V100> : &k_tarch_pool<128, V100>;
    hipLaunchKernelGGL(fn, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, L.z, keep, L.creal, scale, out, L.arg, n, L.h, L.w);
}

// z -> a of one block.  train: batch statistics + the dropout masks; eval: running statistics, the caller's masks keep everything
void block_forward(ArchTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* keep, float scale, bool train) {
    const int i = L.slot / 6;
    const uint8_t* kp = keep + (size_t)n * KEEP_OFF[i];
    if (!t->bn) { launch_pool<true>(s, L, kp, scale, L.a, n); return; }
    launch_pool<false>(s, L, nullptr, 1.f, L.pl, n);
    float* mean = t->stat + i * 512;
    float* invstd = mean + 128;
    const int hw = (L.h / 2) * (L.w / 2);
    const size_t rows = (size_t)n * hw;
    if (train) {
        t_bn_stats(s, L.C, L.pl, rows, t->red);
        t_fin_bn_stats(s, t->red, T_RED_BLOCKS, L.C, (double)rows, t->p.bn_momentum, mean, invstd, t->param(L.slot + K_RM), t->param(L.slot + K_RV), t->bad_target);
    } else {
        t_bn_from_running(s, t->param(L.slot + K_RM), t->param(L.slot + K_RV), L.C, mean, invstd);
    }
    const size_t lanes = rows * (L.C / 4);
    const auto fn = L.C == 16 ? &k_tarch_bn_apply<16> : L.C == 64 ? &k_tarch_bn_apply<64> : &k_tarch_bn_apply<128>;
    hipLaunchKernelGGL(fn, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, L.pl, mean, invstd, t->param(L.slot + K_G), t->param(L.slot + K_BE), kp, L.creal, scale,
                       L.a, rows, hw);
}

// da -> dz written over z, the gradients of bias (and gamma, beta); then the weight gradient and the data gradient of blocks 2 and 3
void block_backward(ArchTrainer* t, hipStream_t s, const Block& L, int n, const uint8_t* keep, float scale) {
    const int i = L.slot / 6;
    const uint8_t* kp = keep + (size_t)n * KEEP_OFF[i];
    float* mean = t->stat + i * 512;
    float* invstd = mean + 128;
    float* sums = mean + 256;
    const int hw = (L.h / 2) * (L.w / 2);
    const size_t rows = (size_t)n * hw;
    if (t->bn) {
        const auto fn = L.C == 16 ? &k_tarch_bn_bwd_stats<16> : L.C == 64 ? &k_tarch_bn_bwd_stats<64> : &k_tarch_bn_bwd_stats<128>;
        hipLaunchKernelGGL(fn, dim3(T_RED_BLOCKS), dim3(256), 0, s, L.da, L.pl, mean, invstd, t->param(L.slot + K_G), t->param(L.slot + K_BE), kp, L.creal, scale, rows, hw,
                           t->red);
        t_fin_bn_bwd(s, t->red, T_RED_BLOCKS, L.C, sums, t->grad(L.slot + K_G), t->grad(L.slot + K_BE));
    }
    {
        const size_t total = (size_t)n * ((L.h + 1) / 2) * ((L.w + 1) / 2) * (L.C / 4);
        // whole rounds: every workgroup takes the same number of elements
        const size_t nb0 = (total + 255) / 256, per = (nb0 + T_BWD_BLOCKS - 1) / T_BWD_BLOCKS, nb = (nb0 + per - 1) / per;
        const float inv_count = (float)(1.0 / (double)std::max<size_t>(rows, 1));
        if (t->bn) {
            const auto fn = L.C == 16 ? &k_tarch_unpool<16, false> : L.C == 64 ? &k_tarch_unpool<64, false> : &k_tarch_unpool<128, false>;
            hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(256), 0, s, L.da, L.pl, L.arg, L.z, mean, invstd, t->param(L.slot + K_G), t->param(L.slot + K_BE), kp, L.creal, scale,
                               sums, inv_count, n, L.h, L.w, t->red_bias);
        } else {
            const auto fn = L.C == 16 ? &k_tarch_unpool<16, true> : L.C == 64 ? &k_tarch_unpool<64, true> : &k_tarch_unpool<128, true>;
            hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(256), 0, s, L.da, nullptr, L.arg, L.z, nullptr, nullptr, nullptr, nullptr, kp, L.creal, scale, nullptr, 0.f, n, L.h,
                               L.w, t->red_bias);
        }
        t_fin_bias(s, t->red_bias, (int)nb, L.C, t->grad(L.slot + K_B));
    }
    if (i == 0) return;
    const Block& below = t->L[i - 1];
    tany_wgrad(s, t->geom, i, n, below.a, L.z, t->part);
    t_wgrad_reduce(s, t->part, t->geom.wg_shares(i, n), L.CI, L.C, L.cic, t->grad(L.slot + K_W));
    t_repack_bwd(s, t->param(L.slot + K_W), L.CI, L.C, L.cic, L.dg_co, L.dg_cic, L.wb);
    tany_conv_dgrad(s, t->geom, i, n, L.z, L.wb, below.da);
}

// forward pass up to the per-sample loss / arg-max and the gradient at the ReLU's input of the head (k_tarch_head); probs: a prediction
void trainer_forward(ArchTrainer* t, hipStream_t s, const float* x, const int32_t* targets, int n, const uint8_t* keep, const float* scale, bool train, float* probs = nullptr) {
    Block* L = t->L;
    tany_conv1(s, t->geom, n, x, t->param(K_W), t->param(K_B), L[0].z);
    block_forward(t, s, L[0], n, keep, scale[0], train);
    for (int i = 1; i < 3; ++i) {
        tany_conv_fwd(s, t->geom, i, n, L[i - 1].a, t->param(L[i].slot + K_W), t->param(L[i].slot + K_B), L[i].z);
        block_forward(t, s, L[i], n, keep, scale[i], train);
    }
    tany_fc1(s, t->geom, n, L[2].a, t->param(S_F1W), t->hpart, t->hsum);
    float* mean = t->stat + 3 * 512;
    float* invstd = mean + 128;
    const uint8_t* kp = keep + (size_t)n * KEEP_OFF[3];
    if (t->bn) {
        if (train) hipLaunchKernelGGL(k_tarch_bn1d_stats, dim3(1), dim3(128), 0, s, t->hsum, t->param(S_F1B), n, t->p.bn_momentum, mean, invstd, t->param(S_RM4), t->param(S_RV4), t->bad_target);
        else t_bn_from_running(s, t->param(S_RM4), t->param(S_RV4), HID, mean, invstd);
        hipLaunchKernelGGL(k_tarch_head<true>, dim3(n), dim3(128), 0, s, t->hsum, n, t->param(S_F1B), mean, invstd, t->param(S_G4), t->param(S_BE4), kp, scale[3], t->param(S_F2W),
                           t->param(S_F2B), targets, t->classes, t->xhat, t->hd, t->dl, t->dy, t->loss, t->correct, probs);
    } else {
        tarch_head_plain(s, t->hsum, n, t->param(S_F1B), kp, scale[3], t->param(S_F2W), t->param(S_F2B), targets, t->classes, t->hd, t->dl, t->dh, t->loss, t->correct, probs);
    }
}

// steps with a target outside 0..classes-1 were refused on the device (k_t_check_targets): train.hip's rule and texts
int check_targets(ArchTrainer* t) {
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

int fetch_loss(ArchTrainer* t, hipStream_t s, float* h_loss, int32_t* h_correct) {
    float two[2];
    TH_CHECK_HIP(hipMemcpyAsync(two, t->out2, sizeof(two), hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    if (h_loss) *h_loss = two[0];
    if (h_correct) *h_correct = (int32_t)two[1];
    return check_targets(t);
}

constexpr float ONES[4] = {1.f, 1.f, 1.f, 1.f};

int stage(ArchTrainer* t, const char* who, const float* inputs, const int32_t* targets, int n, const uint8_t* keep_masks) {
    for (int i = 0; i < n; ++i)
        if (targets[i] < 0 || targets[i] >= t->classes) { set_error(std::string(who) + ": target class out of range"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(t->ctx->p.device));
    hipStream_t s = t->ctx->stream;
    TH_CHECK_HIP(hipMemcpyAsync(t->x_stage, inputs, (size_t)n * t->H * t->W * t->CH * sizeof(float), hipMemcpyHostToDevice, s));
    TH_CHECK_HIP(hipMemcpyAsync(t->y_stage, targets, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (keep_masks) TH_CHECK_HIP(hipMemcpyAsync(t->keep_stage, keep_masks, (size_t)n * KEEP_ROW, hipMemcpyHostToDevice, s));
    return TREXHIP_OK;
}

}  // namespace

int arch_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* p, ArchTrainer** out) {
    const char* who = "trexhip_trainer_create";
    ArchBlob ab;
    if (const int rc = parse_arch_blob(blob, bytes, who, &ab)) return rc;
    if (ab.id != TREXHIP_NET_V100 && ab.id != TREXHIP_NET_V110) { set_error(std::string(who) + ": this version does not train"); return TREXHIP_E_UNSUPPORTED; }
    if (hipSetDevice(ctx->p.device) != hipSuccess) { set_error("trexhip_trainer_create: hipSetDevice failed"); return TREXHIP_E_DEVICE; }
    ArchTrainer* t = new ArchTrainer();
    t->ctx = ctx; t->version = ab.id; t->bn = ab.id == TREXHIP_NET_V110; t->classes = ab.classes; t->CH = ab.CH; t->max_n = p->max_batch; t->p = *p;
    t->W = ab.W; t->H = ab.H;
    t->geom = train_any_geom(ab.W, ab.H, ab.CH);
    const size_t P = t->geom.P;
    // ---- the tensors: torch's count, the count held (block 3 and fc1 padded to 128 channels), the version's state_dict order
    const float* src[S_COUNT] = {};
    for (int i = 0; i < 3; ++i) {
        const size_t ci_r = i ? CR[i - 1] : ab.CH, ci_p = i ? CP[i - 1] : ab.CH;
        t->cnt[6 * i] = (size_t)CR[i] * ci_r * 25; t->isz[6 * i] = (size_t)CP[i] * ci_p * 25;
        for (int k = 1; k < 6; ++k) { t->cnt[6 * i + k] = CR[i]; t->isz[6 * i + k] = CP[i]; }
        for (int k = 0; k < 6; ++k) src[6 * i + k] = ab.conv[i][k];
    }
    t->cnt[S_F1W] = (size_t)HID * 100 * P; t->isz[S_F1W] = t->geom.fc1_weight_floats();
    for (int k = S_F1B; k <= S_RV4; ++k) t->cnt[k] = t->isz[k] = HID;
    t->cnt[S_F2W] = t->isz[S_F2W] = (size_t)ab.classes * HID; t->cnt[S_F2B] = t->isz[S_F2B] = ab.classes;
    src[S_F1W] = ab.fc1w; src[S_F1B] = ab.fc1b; src[S_F2W] = ab.fc2w; src[S_F2B] = ab.fc2b;
    for (int k = 0; k < 4; ++k) src[S_G4 + k] = ab.bn1d[k];
    size_t at = 0;
    for (int k = 0; k < S_COUNT; ++k) {
        const bool is_bn = (k < 18 && k % 6 >= 2) || (k >= S_G4 && k <= S_RV4);
        if (is_bn && !t->bn) t->cnt[k] = t->isz[k] = 0;
        else t->order[t->n_tensors++] = k;
        t->off[k] = at;
        at += (t->isz[k] + 63) / 64 * 64;
    }
    t->off[S_COUNT] = at; t->total = at;
    Block* L = t->L;
    for (int i = 0; i < 3; ++i) { L[i].C = CP[i]; L[i].CI = i ? CP[i - 1] : ab.CH; L[i].creal = CR[i]; L[i].h = t->geom.L[i].h; L[i].w = t->geom.L[i].w; L[i].slot = 6 * i; }
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
        TRY(t->mem.device(&L[i].arg, pooled / 4, who));
        if (t->bn) TRY(t->mem.device(&L[i].pl, pooled, who));
    }
    TRY(t->mem.device(&L[2].wb, (size_t)4 * 25 * 32 * 64, who)); TRY(t->mem.device(&L[1].wb, (size_t)2 * 25 * 32 * 32, who));
    TRY(t->mem.device(&t->part, t->geom.part_floats(), who)); TRY(t->mem.device(&t->part1, t->geom.part1_floats(n), who));
    TRY(t->mem.device(&t->red_bias, (size_t)T_BWD_BLOCKS * 128, who)); TRY(t->mem.device(&t->red, (size_t)T_BWD_BLOCKS * 2 * 128, who));
    TRY(t->mem.device(&t->stat, (size_t)4 * 512, who));
    TRY(t->mem.device(&t->hpart, t->geom.hpart_floats(n), who)); TRY(t->mem.device(&t->hsum, n * HID, who)); TRY(t->mem.device(&t->xhat, n * HID, who));
    TRY(t->mem.device(&t->hd, n * HID, who)); TRY(t->mem.device(&t->dl, n * ab.classes, who)); TRY(t->mem.device(&t->dy, n * HID, who)); TRY(t->mem.device(&t->dh, n * HID, who));
    TRY(t->mem.device(&t->loss, n, who)); TRY(t->mem.device(&t->correct, n, who)); TRY(t->mem.device(&t->out2, 2, who)); TRY(t->mem.device(&t->bad_target, 2, who));
    TRY(t->mem.device(&t->keep, n * KEEP_ROW, who)); TRY(t->mem.device(&t->keep_stage, n * KEEP_ROW, who));
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

// the BatchNorm-free head as another chain launches it (train_cat.hip): k_tarch_head<false> and k_tarch_head_grads, stated here once
void tarch_head_plain(hipStream_t s, const float* hsum, int n, const float* b1, const uint8_t* keep, float scale, const float* w2, const float* b2, const int32_t* targets,
                      int classes, float* hd, float* dl, float* dh, float* loss, int32_t* correct, float* probs) {
    hipLaunchKernelGGL(k_tarch_head<false>, dim3(n), dim3(128), 0, s, hsum, n, b1, nullptr, nullptr, nullptr, nullptr, keep, scale, w2, b2, targets, classes, nullptr, hd, dl, dh,
                       loss, correct, probs);
}
void tarch_head_grads(hipStream_t s, const float* dl, const float* hd, const float* dh, int n, int classes, float* g_w2, float* g_b2, float* g_b1) {
    hipLaunchKernelGGL(k_tarch_head_grads, dim3((classes * HID + classes + HID + 255) / 256), dim3(256), 0, s, dl, hd, dh, n, classes, g_w2, g_b2, g_b1);
}

void arch_trainer_destroy(ArchTrainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->p.device);
    (void)hipStreamSynchronize(t->ctx->stream);
    trainer_free(t);
}

size_t arch_trainer_keep_mask_bytes(int n) { return (size_t)n * KEEP_ROW; }
void arch_trainer_set_lr(ArchTrainer* t, float lr) { t->p.lr = lr; }
int64_t arch_trainer_steps(const ArchTrainer* t) { return t->step; }
void arch_trainer_info(const ArchTrainer* t, int32_t* width, int32_t* height, int32_t* version, int32_t* max_batch) {
    if (width) *width = t->W;
    if (height) *height = t->H;
    if (version) *version = t->version;
    if (max_batch) *max_batch = t->max_n;
}

int arch_trainer_step(ArchTrainer* t, bool host, const float* x, const int32_t* targets, int n, const uint8_t* d_keep, float* h_loss, int32_t* h_correct) {
    const char* who = host ? "trexhip_train_step" : "trexhip_train_step_device";
    // BatchNorm over one value per channel: the reference raises "Expected more than 1 value per channel when training"
    if (t->bn && n < 2) { set_error(std::string(who) + ": a v110 training step needs n >= 2 (BatchNorm1d over the batch: more than 1 value per channel)"); return TREXHIP_E_INVALID; }
    if (host) {
        if (const int rc = stage(t, who, x, targets, n, d_keep)) return rc;
        x = t->x_stage; targets = t->y_stage;
        if (d_keep) d_keep = t->keep_stage;
    }
    TH_CHECK_HIP(hipSetDevice(t->ctx->p.device));
    hipStream_t s = t->ctx->stream;
    const float* rate = P_DROP[t->bn ? 1 : 0];
    float scale[4];
    for (int i = 0; i < 4; ++i) scale[i] = 1.0f / (1.0f - rate[i]);
    const uint8_t* keep = d_keep;
    if (!keep) {
        // the first three planes share a rate; the head's plane is drawn from another stream of the same counter hash
        t_masks(s, t->keep, (size_t)n * KEEP_OFF[3], t->p.seed, (uint64_t)t->step, rate[0]);
        t_masks(s, t->keep + (size_t)n * KEEP_OFF[3], (size_t)n * HID, t->p.seed ^ 0xD1B54A32D192ED03ull, (uint64_t)t->step, rate[3]);
        keep = t->keep;
    }
    t_check_targets(s, targets, n, t->classes, t->bad_target, 0);
    trainer_forward(t, s, x, targets, n, keep, scale, true);
    // ---- backward
    if (t->bn) {
        float* mean = t->stat + 3 * 512;
        hipLaunchKernelGGL(k_tarch_bn1d_sums, dim3(1), dim3(128), 0, s, t->dy, t->xhat, n, mean + 256, t->grad(S_G4), t->grad(S_BE4));
        hipLaunchKernelGGL(k_tarch_bn1d_dh, dim3((n * HID + 255) / 256), dim3(256), 0, s, t->dy, t->xhat, mean + 256, t->param(S_G4), mean + 128, n, t->dh);
    }
    tarch_head_grads(s, t->dl, t->hd, t->dh, n, t->classes, t->grad(S_F2W), t->grad(S_F2B), t->grad(S_F1B));
    tany_fc1_wgrad(s, t->geom, n, t->L[2].a, t->dh, t->grad(S_F1W));
    t_loss(s, t->loss, t->correct, n, t->out2);
    tany_fc1_dgrad(s, t->geom, n, t->dh, t->param(S_F1W), t->L[2].da);
    for (int i = 2; i >= 0; --i) block_backward(t, s, t->L[i], n, keep, scale[i]);
    tany_wgrad1(s, t->geom, n, x, t->L[0].z, t->part1);
    t_reduce(s, t->part1, n * t->geom.wg1_tiles, t->CH * 400, t->grad(K_W));
    // ---- optimizer
    t->step += 1;
    {
        uint32_t lo[4], hi[4];                                   // running statistics are buffers: mean and variance of a BatchNorm lie side by side
        int k = 0;
        if (t->bn)
            for (int rm : {(int)K_RM, 6 + K_RM, 12 + K_RM, (int)S_RM4}) { lo[k] = (uint32_t)t->off[rm]; hi[k] = (uint32_t)(t->off[rm + 1] + t->isz[rm + 1]); ++k; }
        t_adam(s, t->P, t->G, t->M, t->V, t->total, lo, hi, k, t->p.lr, t->p.beta1, t->p.beta2, t->p.eps, t->step, t->bad_target);
    }
    TH_CHECK_HIP(hipGetLastError());
    if (h_loss || h_correct) { if (const int rc = fetch_loss(t, s, h_loss, h_correct)) return rc; }
    if (host) TH_CHECK_HIP(hipStreamSynchronize(s));             // the caller's buffers may go away
    return TREXHIP_OK;
}

int arch_trainer_eval(ArchTrainer* t, bool host, const float* x, const int32_t* targets, int n, float* h_loss, int32_t* h_correct) {
    if (host) {
        if (const int rc = stage(t, "trexhip_train_eval", x, targets, n, nullptr)) return rc;
        x = t->x_stage; targets = t->y_stage;
    }
    TH_CHECK_HIP(hipSetDevice(t->ctx->p.device));
    hipStream_t s = t->ctx->stream;
    TH_CHECK_HIP(hipMemsetAsync(t->keep, 1, (size_t)n * KEEP_ROW, s));                 // nothing dropped
    t_check_targets(s, targets, n, t->classes, t->bad_target, 1);
    trainer_forward(t, s, x, targets, n, t->keep, ONES, false);
    t_loss(s, t->loss, t->correct, n, t->out2);
    TH_CHECK_HIP(hipGetLastError());
    return fetch_loss(t, s, h_loss, h_correct);
}

int arch_trainer_predict(ArchTrainer* t, const uint8_t* d_crops, int n, float* d_probs) {
    trexhip_ctx* ctx = t->ctx;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    TH_CHECK_HIP(hipMemsetAsync(t->keep, 1, (size_t)std::min(n, t->max_n) * KEEP_ROW, s));       // nothing dropped
    for (int at = 0; at < n; at += t->max_n) {
        const int m = std::min(t->max_n, n - at);
        const int rc = trexhip_augment_device(ctx, nullptr, d_crops + (size_t)at * t->H * t->W * t->CH, nullptr, m, nullptr, m, t->W, t->H, t->CH, nullptr, 0, 0, t->x_stage, nullptr);
        if (rc != TREXHIP_OK) return rc;
        trainer_forward(t, s, t->x_stage, nullptr, m, t->keep, ONES, false, d_probs + (size_t)at * t->classes);
    }
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

int arch_trainer_read(ArchTrainer* t, int32_t tensor, int32_t kind, float* out, size_t count) {
    if (!out || tensor < 0 || tensor >= t->n_tensors || kind < 0 || kind > 3) { set_error("trexhip_trainer_read: bad argument"); return TREXHIP_E_INVALID; }
    const int slot = t->order[tensor];
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

int arch_trainer_export(ArchTrainer* t, void* blob, size_t capacity, size_t* bytes) {
    const size_t need = arch_blob_bytes(t->version, t->classes, t->CH, t->W, t->H);
    if (bytes) *bytes = need;
    if (capacity < need) { set_error("trexhip_trainer_export: buffer too small (the bytes of the blob the trainer was created from)"); return TREXHIP_E_CAPACITY; }
    write_weight_blob_header(blob, t->classes, t->W, t->H, t->CH);
    static_cast<int32_t*>(blob)[6] = t->version;
    float* dst = reinterpret_cast<float*>(static_cast<char*>(blob) + 32);
    for (int k = 0; k < t->n_tensors; ++k) {
        const size_t cnt = t->cnt[t->order[k]];
        if (const int rc = arch_trainer_read(t, k, 0, dst, cnt)) return rc;
        dst += cnt;
    }
    return TREXHIP_OK;
}

}  // namespace trexhip
