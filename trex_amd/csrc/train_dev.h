// train_dev.h -- the device helpers that the training kernels of train.hip (k_t_bn_stats) and the size-following ones (train_any.hip,
// train_arch.hip) share: the pool's backward rule and the fixed-order column sums of a workgroup.  One statement of each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace trexhip {

// a block's column sums: the RL row-lanes of every channel added in fixed order -> partial[block][plane][C]
template <int C, int NP>
__device__ __forceinline__ void block_columns(const double (&acc)[NP][4], double* sh /*[256 / (C / 4) * C]*/, double* partial) {
    constexpr int LC = C / 4, RL = 256 / LC;
    const int tid = threadIdx.x, cl = tid % LC, rl = tid / LC;
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[rl * C + cl * 4 + k] = acc[pl][k];
        __syncthreads();
        if (tid < C) {
            double t = 0;
            for (int r = 0; r < RL; ++r) t += sh[r * C + tid];
            partial[((size_t)blockIdx.x * NP + pl) * C + tid] = t;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ float f4get(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ void f4set(float4& v, int k, float x) { if (k == 0) v.x = x; else if (k == 1) v.y = x; else if (k == 2) v.z = x; else v.w = x; }

// the gradient that reaches the BN output of one pooled element: through dropout, the pool's arg-max (first maximum in scan order,
// like torch's max_pool2d) and the ReLU gate.  Returns the arg-max position and x-hat there.
__device__ __forceinline__ float pooled_grad(const float zq[4], float mean, float inv, float alpha, float beta, float da, bool kept, float scale,
                                             int* arg, float* xhat) {
    float best = zq[0] * alpha + beta;
    int bi = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        const float y = zq[q] * alpha + beta;
        if (y > best) { best = y; bi = q; }
    }
    *arg = bi;
    *xhat = (zq[bi] - mean) * inv;
    return (kept && best > 0.f) ? da * scale : 0.f;
}

}  // namespace trexhip
