// cnn.hip -- identity network V118_3 forward + softmax on gfx950 (fp32-class arithmetic, MFMA for the convs).
//
// Replaces VINetwork::probabilities -> Python predict() -> predict_numpy
//   Application/src/tracker/ml/VisualIdentification.cpp:440-485
//   Application/src/tracker/python/visual_recognition_torch.py:290-352,984-1034
// for the network visual_identification_network_torch.py:184-258 (V118_3, eval mode):
//   x = float(u8)  ->  [conv5x5 same -> BN -> ReLU -> maxpool2] x3 -> flatten(NCHW) -> fc1(12800->100)
//   -> LayerNorm(100) -> ReLU -> fc2(100->classes) -> softmax.
//
// Default chain (1-channel crops, fp16 two-piece split): k_conv12_rs (cnn_fused12rs.h) or k_conv12_wpre (cnn_fused12.h): conv1 inside conv2 -> V3
// -> k_conv5_wpair (cnn_conv3p.h) -> k_fc1_split -> k_head.  The kernels of this file are the exact-fp32 / bf16 precision modes, the fallbacks and the head:
// Kernels (DESIGN.md "Identity network"):
//   k_conv1     C_in=1: VALU, one block per crop, u8 crop staged in LDS, fused BN+ReLU+pool
//   k_conv5<>   conv2/conv3 as 25 shifted GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32):
//               input patch (+2 halo) of one ci-chunk staged once in LDS, A fragments read from it at
//               the tap's offset (no im2col), weights per (tap, ci-chunk) double-buffered in LDS,
//               pixels ordered pool-window-major so the 2x2 max-pool is a max over 4 accumulator
//               registers of one lane; BN folded into weights/bias; epilogue bias+ReLU+pool
//   k_fc1       [crops x 12800] x [12800 x 128] MFMA GEMM, LDS tiles
//   k_head      LayerNorm + ReLU + fc2 + softmax, four crops per wave
#include "cnn_net.h"
#include "cnn_arch.h"
#include "cnn_split.h"
#include "conv_tiled.h"
#include "cnn_weights.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace trexhip {

// ------------------------------------------------------------------------------------------------
// conv1: 1 -> 16 channels, 80x80 -> pooled 40x40x16 (NHWC fp32)
// ------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(256, 2) void k_conv1(const uint8_t* __restrict__ crops, const float* __restrict__ w /*[CH][25][16]*/,
                                                  const float* __restrict__ bias /*[16]*/, float* __restrict__ out, int S) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int PW = S + 4;
    float* wl = lds;                        // [CH*25*16]  (first: 16-byte aligned for float4 reads)
    float* img = lds + CH * 25 * 16;        // [CH][PW*PW]
    const int crop = blockIdx.x;
    const uint8_t* src = crops + (size_t)crop * S * S * CH;
    for (int i = threadIdx.x; i < CH * PW * PW; i += 256) img[i] = 0.f;
    for (int i = threadIdx.x; i < CH * 25 * 16; i += 256) wl[i] = w[i];
    __syncthreads();
    for (int i = threadIdx.x; i < S * S * CH; i += 256) {
        const int c = i % CH, p = i / CH, y = p / S, x = p - y * S;
        img[c * PW * PW + (y + 2) * PW + x + 2] = (float)src[i];       // predict_numpy: float32(u8), no scaling
    }
    __syncthreads();
    const int HW = S / 2;
    for (int wi = threadIdx.x; wi < HW * HW; wi += 256) {
        const int wy = wi / HW, wx = wi - wy * HW;
        float acc[4][16];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int co = 0; co < 16; ++co) acc[s4][co] = 0.f;
        for (int c = 0; c < CH; ++c) {
            const float* base = img + c * PW * PW + (2 * wy) * PW + 2 * wx;
#pragma unroll 1
            for (int ky = 0; ky < 5; ++ky) {
                float r0[6], r1[6];                                     // two input rows feed output rows 0 and 1 of the window
#pragma unroll
                for (int b6 = 0; b6 < 6; ++b6) { r0[b6] = base[ky * PW + b6]; r1[b6] = base[(ky + 1) * PW + b6]; }
#pragma unroll
                for (int kx = 0; kx < 5; ++kx) {
                    const float4* wt = reinterpret_cast<const float4*>(wl + (c * 25 + ky * 5 + kx) * 16);
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const float4 wv = wt[q4];
                        const float ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int co = q4 * 4 + q;
                            acc[0][co] = fmaf(r0[kx], ww[q], acc[0][co]);
                            acc[1][co] = fmaf(r0[kx + 1], ww[q], acc[1][co]);
                            acc[2][co] = fmaf(r1[kx], ww[q], acc[2][co]);
                            acc[3][co] = fmaf(r1[kx + 1], ww[q], acc[3][co]);
                        }
                    }
                }
            }
        }
        float* o = out + ((size_t)crop * HW * HW + wi) * 16;
#pragma unroll
        for (int co = 0; co < 16; co += 4) {
            float4 v;
            float* vv = &v.x;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float m = fmaxf(fmaxf(acc[0][co + q], acc[1][co + q]), fmaxf(acc[2][co + q], acc[3][co + q]));
                vv[q] = fmaxf(m + bias[co + q], 0.f);
            }
            *reinterpret_cast<float4*>(o + co) = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// conv1 on the matrix cores (1 input channel): the u8 crop is exact in fp16, the folded weights are split into two fp16
// pieces (scaled by a power of two), so two v_mfma_f32_16x16x32_f16 products per term are fp32-class.
//   M (16 rows)  = 8 windows x 2 image rows; a window is 8 consecutive padded pixels starting at x4 = 0,4,8,...
//   K (32)       = 4 kernel rows x 8 window slots (second MFMA: kernel row 4, the other 24 k are zero weights)
//   N (16)       = output channels
// One A fragment serves the four outputs x4+s, s = 0..3, through four weight matrices with the taps shifted by s slots
// (slot = kx + s <= 7), so every LDS read starts at a multiple of 4 pixels (8-byte aligned).  The accumulator layout
// (lane: column co, rows 4g..4g+3 = two windows x two image rows) makes the 2x2 max-pool a max over registers of one lane.
// ------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// the fp16 range guard's plan: guard_plan (conv_tiled.h), by a launch of its own or by the small head's first workgroup
__device__ __forceinline__ int fb_count(const uint32_t* __restrict__ plan, const int n) { return (plan && plan[1] == 1u) ? (int)plan[0] : n; }
__global__ __launch_bounds__(1024) void k_guard_plan(uint32_t* __restrict__ overflow, uint8_t* __restrict__ flags, const int n, uint32_t* __restrict__ plan) {
    __shared__ uint32_t cnt;
    guard_plan<1024>(overflow, flags, n, plan, cnt);
}

__global__ __launch_bounds__(256) void k_conv1_mfma(const uint8_t* __restrict__ crops, const uint4* __restrict__ wtab /*[16][64]*/,
                                                    const float* __restrict__ bias, float* __restrict__ out, const float inv_scale,
                                                    const uint32_t* __restrict__ guard) {
    if (guard && guard[1] == 0u) return;                    // guarded re-run of the default chain (guard = the plan of k_guard_plan): nothing to do unless the fp16 range flag is up
    if ((int)blockIdx.x >= fb_count(guard, (int)gridDim.x)) return;
    constexpr int S = 80, PH = 84, PITCH = 88;              // halves per padded row (176 B: rows land on distinct bank groups)
    __shared__ __attribute__((aligned(16))) _Float16 img[PH * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int crop = plan_crop(guard, (int)blockIdx.x);
    const uint8_t* src = crops + (size_t)crop * S * S;
    // zero the padded image, then 16 pixels per thread: one 16-byte load of the crop row, 16 halves into LDS
    for (int i = tid; i < PH * PITCH * 2 / 16; i += 256) reinterpret_cast<uint4*>(img)[i] = make_uint4(0, 0, 0, 0);
    __shared__ __attribute__((aligned(16))) float tr[4][64 * 17];      // per-wave transpose buffer of the epilogue
    __syncthreads();
    for (int i = tid; i < S * S / 16; i += 256) {
        const int y = i / (S / 16), c16 = (i - y * (S / 16)) * 16;
        const uint4 v = reinterpret_cast<const uint4*>(src)[i];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        uint32_t* d = reinterpret_cast<uint32_t*>(img + (y + 2) * PITCH + 2 + c16);     // 4-byte aligned (2 + c16 is even)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t b0 = (w4[k >> 1] >> (16 * (k & 1))) & 0xffu, b1 = (w4[k >> 1] >> (16 * (k & 1) + 8)) & 0xffu;
            const _Float16 h0 = (_Float16)(float)b0, h1 = (_Float16)(float)b1;
            d[k] = (uint32_t)__builtin_bit_cast(uint16_t, h0) | ((uint32_t)__builtin_bit_cast(uint16_t, h1) << 16);
        }
    }
    uint4 bf[16];
#pragma unroll
    for (int f = 0; f < 16; ++f) bf[f] = wtab[f * 64 + lane];
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    const int co = r;
    const float bz = bias[co];
    float* oc = out + (size_t)crop * 40 * 40 * 16;
    for (int tile = wave; tile < 100; tile += 4) {
        const int wdx = tile * 8 + (r >> 1);
        const int yp = wdx / 20, x4 = (wdx - yp * 20) * 4;
        const int row = 2 * yp + (r & 1);
        const _Float16* p1 = img + (row + q) * PITCH + x4;
        const _Float16* p2 = img + (row + 4) * PITCH + x4;
        uint4 a1u, a2u;
        { const uint2 lo = *reinterpret_cast<const uint2*>(p1), hi = *reinterpret_cast<const uint2*>(p1 + 4); a1u = make_uint4(lo.x, lo.y, hi.x, hi.y); }
        { const uint2 lo = *reinterpret_cast<const uint2*>(p2), hi = *reinterpret_cast<const uint2*>(p2 + 4); a2u = make_uint4(lo.x, lo.y, hi.x, hi.y); }
        const f16x8 a1 = __builtin_bit_cast(f16x8, a1u), a2 = __builtin_bit_cast(f16x8, a2u);
        f32x4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, __builtin_bit_cast(f16x8, bf[s * 4 + 1]), c, 0, 0, 0);   // low pieces first
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, __builtin_bit_cast(f16x8, bf[s * 4 + 3]), c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, __builtin_bit_cast(f16x8, bf[s * 4 + 0]), c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, __builtin_bit_cast(f16x8, bf[s * 4 + 2]), c, 0, 0, 0);
            acc[s] = c;
        }
        // lane (co, q) holds 4 consecutive pooled pixels of channel co; through LDS to one float4 (4 channels of one pixel) per lane
        float* tw = tr[wave];
#pragma unroll
        for (int pos = 0; pos < 2; ++pos) {
            const float m0 = fmaxf(fmaxf(acc[0][2 * pos], acc[0][2 * pos + 1]), fmaxf(acc[1][2 * pos], acc[1][2 * pos + 1]));
            const float m1 = fmaxf(fmaxf(acc[2][2 * pos], acc[2][2 * pos + 1]), fmaxf(acc[3][2 * pos], acc[3][2 * pos + 1]));
            tw[(4 * q + 2 * pos) * 17 + co] = fmaxf(m0 * inv_scale + bz, 0.f);
            tw[(4 * q + 2 * pos + 1) * 17 + co] = fmaxf(m1 * inv_scale + bz, 0.f);
        }
        __builtin_amdgcn_wave_barrier();
        {
            const int px = lane >> 2, c4 = (lane & 3) * 4;                 // 16 pooled pixels x 4 channel quads
            const float* s = tw + px * 17 + c4;
            const float4 v = make_float4(s[0], s[1], s[2], s[3]);
            *reinterpret_cast<float4*>(oc + ((size_t)tile * 16 + px) * 16 + c4) = v;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// the same for 3-channel crops (meta_encoding rgb8): one fp16 plane per channel in LDS; per shift four MFMAs of K = 32:
// channel 0 / 1 / 2 with kernel rows 0..3, and a fourth whose k-octets 0..2 hold kernel row 4 of the three channels
__global__ __launch_bounds__(256) void k_conv1_mfma3(const uint8_t* __restrict__ crops /*[N][80][80][3]*/, const uint4* __restrict__ wtab /*[32][64]*/,
                                                     const float* __restrict__ bias, float* __restrict__ out, const float inv_scale,
                                                     const uint32_t* __restrict__ guard) {
    if (guard && guard[1] == 0u) return;
    if ((int)blockIdx.x >= fb_count(guard, (int)gridDim.x)) return;
    constexpr int S = 80, PH = 84, PITCH = 88, PLANE = PH * PITCH;
    __shared__ __attribute__((aligned(16))) _Float16 img[3 * PLANE];
    __shared__ __attribute__((aligned(16))) float tr[4][64 * 17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int crop = plan_crop(guard, (int)blockIdx.x);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(crops + (size_t)crop * S * S * 3);
    for (int i = tid; i < 3 * PLANE * 2 / 16; i += 256) reinterpret_cast<uint4*>(img)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    for (int i = tid; i < S * S / 4; i += 256) {               // 4 pixels = 12 bytes = 3 dwords per step
        const int y = i / (S / 4), x = (i - y * (S / 4)) * 4;
        const uint32_t w0 = src[3 * i], w1 = src[3 * i + 1], w2 = src[3 * i + 2];
        const uint32_t by[12] = {w0 & 0xff, (w0 >> 8) & 0xff, (w0 >> 16) & 0xff, w0 >> 24, w1 & 0xff, (w1 >> 8) & 0xff, (w1 >> 16) & 0xff, w1 >> 24,
                                 w2 & 0xff, (w2 >> 8) & 0xff, (w2 >> 16) & 0xff, w2 >> 24};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t* d = reinterpret_cast<uint32_t*>(img + c * PLANE + (y + 2) * PITCH + 2 + x);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const _Float16 h0 = (_Float16)(float)by[(2 * k) * 3 + c], h1 = (_Float16)(float)by[(2 * k + 1) * 3 + c];
                d[k] = (uint32_t)__builtin_bit_cast(uint16_t, h0) | ((uint32_t)__builtin_bit_cast(uint16_t, h1) << 16);
            }
        }
    }
    uint4 bf[32];
#pragma unroll
    for (int f = 0; f < 32; ++f) bf[f] = wtab[f * 64 + lane];
    __syncthreads();
    const int r = lane & 15, q = lane >> 4;
    const int co = r;
    const float bz = bias[co];
    float* oc = out + (size_t)crop * 40 * 40 * 16;
    for (int tile = wave; tile < 100; tile += 4) {
        const int wdx = tile * 8 + (r >> 1);
        const int yp = wdx / 20, x4 = (wdx - yp * 20) * 4;
        const int row = 2 * yp + (r & 1);
        f16x8 a[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            // m < 3: channel m, kernel row q; m == 3: kernel row 4 of channel q (the fourth k-octet meets zero weights)
            const _Float16* pp = m < 3 ? img + m * PLANE + (row + q) * PITCH + x4 : img + (q < 3 ? q : 0) * PLANE + (row + 4) * PITCH + x4;
            const uint2 lo = *reinterpret_cast<const uint2*>(pp), hi = *reinterpret_cast<const uint2*>(pp + 4);
            a[m] = __builtin_bit_cast(f16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
        f32x4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < 4; ++m) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m], __builtin_bit_cast(f16x8, bf[(s * 4 + m) * 2 + 1]), c, 0, 0, 0);   // low pieces first
#pragma unroll
            for (int m = 0; m < 4; ++m) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m], __builtin_bit_cast(f16x8, bf[(s * 4 + m) * 2 + 0]), c, 0, 0, 0);
            acc[s] = c;
        }
        float* tw = tr[wave];
#pragma unroll
        for (int pos = 0; pos < 2; ++pos) {
            const float m0 = fmaxf(fmaxf(acc[0][2 * pos], acc[0][2 * pos + 1]), fmaxf(acc[1][2 * pos], acc[1][2 * pos + 1]));
            const float m1 = fmaxf(fmaxf(acc[2][2 * pos], acc[2][2 * pos + 1]), fmaxf(acc[3][2 * pos], acc[3][2 * pos + 1]));
            tw[(4 * q + 2 * pos) * 17 + co] = fmaxf(m0 * inv_scale + bz, 0.f);
            tw[(4 * q + 2 * pos + 1) * 17 + co] = fmaxf(m1 * inv_scale + bz, 0.f);
        }
        __builtin_amdgcn_wave_barrier();
        {
            const int px = lane >> 2, c4 = (lane & 3) * 4;
            const float* sp = tw + px * 17 + c4;
            *reinterpret_cast<float4*>(oc + ((size_t)tile * 16 + px) * 16 + c4) = make_float4(sp[0], sp[1], sp[2], sp[3]);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// the same convolution on the bf16 matrix cores with fp32-equivalent accuracy (the operand splits: cnn_split.h).  Activations are split while the
// patch is staged (three patches [pixel][16 ci] bf16, 48-byte pixel stride); weights are pre-split on the host (cnn_weights.h: pack_bf16x3).
// ------------------------------------------------------------------------------------------------
template <int CI, int CO, int S, int ROWS, int NTERMS, int CIC = 16>
__global__ __launch_bounds__(512) void k_conv5_split(const float* __restrict__ in /*[N][S][S][CI]*/,
                                                     const uint4* __restrict__ wp /*[CI/16][25][NP][2][CO] x 16 B*/,
                                                     const float* __restrict__ bias, float* __restrict__ out, const float out_scale,
                                                     const uint32_t* __restrict__ guard, const int n_blocks) {
    if (guard && guard[1] == 0u) return;          // re-run pass (guard = the plan of k_guard_plan): only when the fp16 pass flagged an overflow
    using frag = bf16x8;
    using G = ConvGeomB<CI, CO, S, ROWS, SPLIT_NP, CIC>;
    constexpr int Q4 = CIC / 4, KO = CIC / 8;                          // float4 per pixel per chunk, k-octets per chunk
    extern __shared__ __attribute__((aligned(16))) uint8_t ldsb[];
    uint8_t* patch = ldsb;                       // NP pieces
    uint8_t* Bs = ldsb + SPLIT_NP * G::PATCH;    // 2 buffers
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = wave % G::NT, mg = wave / G::NT;
    // grid-stride over the (crop, row band) blocks: the guarded re-run is launched with a small grid, so that the usual case (flag
    // clear, every workgroup returns at once) costs a few microseconds instead of the launch of n * BPC empty workgroups
    const int n_blocks_eff = (guard && guard[1] == 1u) ? (int)guard[0] * G::BPC : n_blocks;      // list mode: the flagged crops only
    for (int blk = blockIdx.x; blk < n_blocks_eff; blk += gridDim.x) {
    if (blk != (int)blockIdx.x) __syncthreads();                      // the previous block's readers are done with the LDS buffers
    const int crop = plan_crop(guard, blk / G::BPC), row0 = (blk % G::BPC) * ROWS;
    constexpr int WR = S / 2;

    int aoff[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int p = (mg + G::WM * m) * 32 + j;
        int off = 0;
        if (p < G::NPIX) {
            const int wi = p >> 2, sub = p & 3;
            const int wy = wi / WR, wx = wi - wy * WR;
            off = ((2 * wy + (sub >> 1)) * G::PW + (2 * wx + (sub & 1))) * G::PSTRIDE;
        }
        aoff[m] = off + h * 16;
    }
    f32x16 acc[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    const float* inc = in + (size_t)crop * S * S * CI;
    constexpr int BV = G::BT / 16;                                      // uint4 per weight tile
    constexpr int BPT = (BV + 511) / 512;
    for (int cc = 0; cc < CI / CIC; ++cc) {
        __syncthreads();
        for (int idx = tid; idx < G::PH * G::PW * Q4; idx += 512) {     // Q4 float4 per pixel
            const int q = idx % Q4, px = idx / Q4;
            const int py = px / G::PW, pxx = px - py * G::PW;
            const int iy = row0 + py - 2, ix = pxx - 2;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (iy >= 0 && iy < S && ix >= 0 && ix < S)
                v = *reinterpret_cast<const float4*>(inc + ((size_t)iy * S + ix) * CI + cc * CIC + q * 4);
            uint32_t a1[4], a2[4], a3[4];
            split3(v.x, a1[0], a2[0], a3[0]); split3(v.y, a1[1], a2[1], a3[1]);
            split3(v.z, a1[2], a2[2], a3[2]); split3(v.w, a1[3], a2[3], a3[3]);
            uint8_t* d = patch + px * G::PSTRIDE + q * 8;
            *reinterpret_cast<uint2*>(d) = make_uint2(a1[0] | (a1[1] << 16), a1[2] | (a1[3] << 16));
            *reinterpret_cast<uint2*>(d + G::PATCH) = make_uint2(a2[0] | (a2[1] << 16), a2[2] | (a2[3] << 16));
            *reinterpret_cast<uint2*>(d + 2 * G::PATCH) = make_uint2(a3[0] | (a3[1] << 16), a3[2] | (a3[3] << 16));
        }
        const uint4* wsrc = wp + (size_t)cc * 25 * BV;
        for (int i = tid; i < BV; i += 512) reinterpret_cast<uint4*>(Bs)[i] = wsrc[i];
        __syncthreads();
        for (int tap = 0; tap < 25; ++tap) {
            const int buf = tap & 1;
            uint4 nb[BPT];
            if (tap < 24) {
#pragma unroll
                for (int u = 0; u < BPT; ++u) { const int i = tid + u * 512; if (i < BV) nb[u] = wsrc[(size_t)(tap + 1) * BV + i]; }
            }
            const int tapoff = ((tap / 5) * G::PW + (tap % 5)) * G::PSTRIDE;
            const uint8_t* asrc = patch + tapoff;
#define LDA(m, piece) __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(asrc + aoff[m] + ks * 32 + (piece) * G::PATCH))
#define MF(a, b, m) acc[m] = mfma16(a, b, acc[m])
#pragma unroll
            for (int ks = 0; ks < CIC / 16; ++ks) {                        // one 16-deep MFMA step per 16 input channels
                const uint8_t* bsrc = Bs + buf * G::BT + ((2 * ks + h) * CO + n * 32 + j) * 16;
                const frag b1 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc));
                const frag b2 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc + KO * CO * 16));
                const frag b3 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc + 2 * KO * CO * 16));
#pragma unroll
                for (int m = 0; m < G::TPW; ++m) {
                    const frag p1 = LDA(m, 0), p2 = LDA(m, 1);
                    if (NTERMS == 6) {
                        const frag p3 = LDA(m, 2);
                        MF(p3, b1, m); MF(p2, b2, m); MF(p1, b3, m);
                    }
                    MF(p2, b1, m); MF(p1, b2, m); MF(p1, b1, m);
                }
            }
#undef LDA
#undef MF
            if (tap < 24) {
#pragma unroll
                for (int u = 0; u < BPT; ++u) { const int i = tid + u * 512; if (i < BV) reinterpret_cast<uint4*>(Bs + (buf ^ 1) * G::BT)[i] = nb[u]; }
            }
            __syncthreads();
        }
    }
    const int co = n * 32 + j;
    const float bz = bias[co];
    float* oc = out + (size_t)crop * WR * WR * CO;
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int mt = mg + G::WM * m;
        if (mt >= G::MT) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int wi = mt * 8 + 2 * g + h;
            if (wi >= G::NPIX / 4) continue;
            const float v = fmaxf(fmaxf(acc[m][4 * g], acc[m][4 * g + 1]), fmaxf(acc[m][4 * g + 2], acc[m][4 * g + 3]));
            const int wy = row0 / 2 + wi / WR, wx = wi % WR;
            oc[((size_t)wy * WR + wx) * CO + co] = fmaxf(v * out_scale + bz, 0.f);     // (out_scale: 1 for the unscaled bf16 weights)
        }
    }
    }
}

// ------------------------------------------------------------------------------------------------
// k_conv5_stream: the fp16 two-piece convolution without a barrier in the tap loop.
//   * weight fragments go global(L2) -> VGPR directly, prefetched two taps ahead (the pre-split weight image is laid out
//     exactly as the MFMA B operand wants it: [chunk][tap][piece][k-octet][co] x 16 B, so a half-wave reads 512 contiguous
//     bytes); nothing but the activation patch lives in LDS, so waves never wait for each other inside a chunk;
//   * with more than one 16-channel chunk the patch is double-buffered and the next chunk is staged (global load, fp16
//     split, LDS store) in slices between the taps of the current one: one barrier per chunk instead of 26;
//   * patch rows are padded so that the row pitch is 8 (mod 16) in 16-byte slots: the 16 lanes of one ds_read_b128 lane
//     group (MI355X guide, LDS table) then hit 16 distinct slots.
// ------------------------------------------------------------------------------------------------
template <int CI, int CO, int S, int ROWS, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_conv5_stream(const float* __restrict__ in /*[N][S][S][CI]*/,
                                                             const uint4* __restrict__ wp /*[CI/16][25][2][2][CO] x 16 B*/,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             const float out_scale, uint32_t* __restrict__ overflow, const int n_units) {
    using G = ConvGeomS<CI, CO, S, ROWS, WAVES>;
    static_assert(G::NCH == 1 || G::NITEMS <= 5, "staging slices do not fit between the taps");
    extern __shared__ __attribute__((aligned(16))) uint8_t ldsb[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = wave % G::NT, mg = wave / G::NT;
    // a unit = ROWS output rows of one crop, one unit per workgroup
    const int unit = blockIdx.x;
    if (unit >= n_units) return;
    constexpr int WR = S / 2;

    int aoff[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int p = (mg + G::WM * m) * 32 + j;
        int off = 0;
        if (p < G::NPIX) {
            const int wi = p >> 2, sub = p & 3;
            const int wy = wi / WR, wx = wi - wy * WR;
            off = (2 * wy + (sub >> 1)) * G::RP + (2 * wx + (sub & 1)) * G::PSTRIDE;
        }
        aoff[m] = off + h * 16;
    }
    const bool last_tile = mg + G::WM * (G::TPW - 1) < G::MT;
    bool ovf = false;
    // one staged item: float4 of 4 input channels of one patch pixel -> two fp16 pieces in LDS
#define STG_LOAD(v_, item_, inc_, row0_, cc_)                                                                                 \
    do {                                                                                                                      \
        const int idx_ = tid + (item_) * G::NTHR;                                                                             \
        v_ = make_float4(0.f, 0.f, 0.f, 0.f);                                                                                 \
        if (idx_ < G::NQ) {                                                                                                   \
            const int px_ = idx_ >> 2, q_ = idx_ & 3;                                                                         \
            const int py_ = px_ / G::PW, pxx_ = px_ - py_ * G::PW;                                                            \
            const int iy_ = (row0_) + py_ - 2, ix_ = pxx_ - 2;                                                                \
            if (iy_ >= 0 && iy_ < S && ix_ >= 0 && ix_ < S)                                                                   \
                v_ = *reinterpret_cast<const float4*>((inc_) + ((size_t)iy_ * S + ix_) * CI + (cc_) * 16 + q_ * 4);           \
        }                                                                                                                     \
    } while (0)
#define STG_STORE(v_, item_, base_)                                                                                           \
    do {                                                                                                                      \
        const int idx_ = tid + (item_) * G::NTHR;                                                                             \
        if (idx_ < G::NQ) {                                                                                                   \
            const int px_ = idx_ >> 2, q_ = idx_ & 3;                                                                         \
            const int py_ = px_ / G::PW, pxx_ = px_ - py_ * G::PW;                                                            \
            uint32_t a1_[4], a2_[4];                                                                                          \
            split2h(v_.x, a1_[0], a2_[0], ovf); split2h(v_.y, a1_[1], a2_[1], ovf);                                           \
            split2h(v_.z, a1_[2], a2_[2], ovf); split2h(v_.w, a1_[3], a2_[3], ovf);                                           \
            uint8_t* d_ = (base_) + py_ * G::RP + pxx_ * G::PSTRIDE + q_ * 8;                                                 \
            *reinterpret_cast<uint2*>(d_) = make_uint2(a1_[0] | (a1_[1] << 16), a1_[2] | (a1_[3] << 16));                     \
            *reinterpret_cast<uint2*>(d_ + G::PATCH) = make_uint2(a2_[0] | (a2_[1] << 16), a2_[2] | (a2_[3] << 16));          \
        }                                                                                                                     \
    } while (0)

    // B fragments of this lane: k-octet h, output channel n*32+j; piece 1 is 2*CO uint4 further
    const uint4* wl = wp + (h * CO + n * 32 + j);
    uint4 bq[5][2];
    bq[0][0] = wl[0]; bq[0][1] = wl[2 * CO];
    bq[1][0] = wl[G::BV]; bq[1][1] = wl[G::BV + 2 * CO];
    const int co = n * 32 + j;
    const float bz = bias[co];
    const int crop = unit / G::BPC, row0 = (unit % G::BPC) * ROWS;
    const float* inc = in + (size_t)crop * S * S * CI;
    for (int it = 0; it < G::NITEMS; ++it) {
        float4 v;
        STG_LOAD(v, it, inc, row0, 0);
        STG_STORE(v, it, ldsb);
    }
    __syncthreads();
    f32x16 acc[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    for (int cc = 0; cc < G::NCH; ++cc) {
        const uint8_t* pbase = ldsb + (G::NBUF > 1 ? (cc & 1) * 2 * G::PATCH : 0);
        uint8_t* nbase = ldsb + (G::NBUF > 1 ? ((cc + 1) & 1) * 2 * G::PATCH : 0);
        const bool more_c = cc + 1 < G::NCH;                             // the next chunk's weights are needed and its patch is staged under this one
        const uint4* wc = wl + (size_t)cc * 25 * G::BV;
        const uint4* wn = wl + (size_t)(cc + 1) * 25 * G::BV;
        float4 sv = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int tap = 0; tap < 25; ++tap) {
            if (tap + 2 < 25) {                // weights two taps ahead (runs into the following chunk's first taps)
                bq[(tap + 2) % 5][0] = wc[(size_t)(tap + 2) * G::BV];
                bq[(tap + 2) % 5][1] = wc[(size_t)(tap + 2) * G::BV + 2 * CO];
            } else if (more_c) {
                bq[(tap + 2) % 5][0] = wn[(size_t)(tap + 2 - 25) * G::BV];
                bq[(tap + 2) % 5][1] = wn[(size_t)(tap + 2 - 25) * G::BV + 2 * CO];
            }
            if (more_c) {
                if (tap % 5 == 0 && tap / 5 < G::NITEMS) STG_LOAD(sv, tap / 5, inc, row0, cc + 1);
                if (tap % 5 == 3 && tap / 5 < G::NITEMS) STG_STORE(sv, tap / 5, nbase);
            }
            const uint8_t* asrc = pbase + ((tap / 5) * G::RP + (tap % 5) * G::PSTRIDE);
            const f16x8 b1 = __builtin_bit_cast(f16x8, bq[tap % 5][0]);
            const f16x8 b2 = __builtin_bit_cast(f16x8, bq[tap % 5][1]);
#pragma unroll
            for (int m = 0; m < G::TPW; ++m) {
                if (m == G::TPW - 1 && !last_tile) continue;       // wave-uniform: this M-group has one tile less
                const f16x8 p1 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(asrc + aoff[m]));
                const f16x8 p2 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(asrc + aoff[m] + G::PATCH));
                acc[m] = mfma16(p2, b1, acc[m]);
                acc[m] = mfma16(p1, b2, acc[m]);
                acc[m] = mfma16(p1, b1, acc[m]);
            }
        }
        if (G::NCH > 1) __syncthreads();
    }
    float* oc = out + (size_t)crop * WR * WR * CO;
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int mt = mg + G::WM * m;
        if (mt >= G::MT) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int wi = mt * 8 + 2 * g + h;
            if (wi >= G::NPIX / 4) continue;
            const float v = fmaxf(fmaxf(acc[m][4 * g], acc[m][4 * g + 1]), fmaxf(acc[m][4 * g + 2], acc[m][4 * g + 3]));
            const int wy = row0 / 2 + wi / WR, wx = wi % WR;
            oc[((size_t)wy * WR + wx) * CO + co] = fmaxf(v * out_scale + bz, 0.f);
        }
    }
#undef STG_LOAD
#undef STG_STORE
    if (__any(ovf) && lane == 0) atomicOr(overflow, 3u);
}

// B^T of F(4,5), points (0, 1, -1, 2, -2, 1/2, -1/2, inf): 8 consecutive inputs -> 8 positions
__device__ __forceinline__ void wino_bt(const float d0, const float d1, const float d2, const float d3, const float d4, const float d5,
                                        const float d6, const float d7, float* __restrict__ u) {
    u[0] = fmaf(5.25f, d2 - d4, d6 - d0);
    u[7] = fmaf(5.25f, d3 - d5, d7 - d1);
    const float e1 = fmaf(-4.25f, d4, d2 + d6), o1 = fmaf(-4.25f, d3, d1 + d5);
    u[1] = e1 + o1; u[2] = e1 - o1;
    const float e2 = fmaf(-1.25f, d4, fmaf(0.25f, d2, d6)), o2 = fmaf(2.f, d5, fmaf(-2.5f, d3, 0.5f * d1));
    u[3] = e2 + o2; u[4] = e2 - o2;
    const float e3 = fmaf(-5.f, d4, fmaf(4.f, d2, d6)), o3 = fmaf(0.5f, d5, fmaf(-2.5f, d3, 2.f * d1));
    u[5] = e3 + o3; u[6] = e3 - o3;
}
// A^T of F(4,5): 8 position sums -> 4 outputs
__device__ __forceinline__ void wino_at(const float m0, const float m1, const float m2, const float m3, const float m4, const float m5,
                                        const float m6, const float m7, float* __restrict__ y) {
    const float e1 = m1 + m2, o1 = m1 - m2, e2 = m3 + m4, o2 = m3 - m4, e3 = m5 + m6, o3 = m5 - m6;
    y[0] = (m0 + e1) + (e2 + e3);
    y[1] = fmaf(0.5f, o3, fmaf(2.f, o2, o1));
    y[2] = fmaf(0.25f, e3, fmaf(4.f, e2, e1));
    y[3] = fmaf(0.125f, o3, fmaf(8.f, o2, o1)) + m7;
}

// ------------------------------------------------------------------------------------------------
// k_conv5_wino: conv 5x5 'same' as a one-dimensional Winograd convolution F(4,5) along x (Cook-Toom, points 0, +-1, +-2, +-1/2, inf),
// direct along y: per kernel row ky, 8 products give 4 neighbouring outputs instead of 20 -> 40 position GEMMs over "tiles"
// (4 outputs in a row) replace 25 tap GEMMs over pixels = 0.4x the matrix work of the direct form.  An exact reformulation
// (visual_identification_network_torch.py:184-258 computes the same sums); measured error ladder in DESIGN.md.
//   * input transform U = B^T d (8 inputs -> 8 positions, fp32 VALU) while a row is staged; each U is then split into two fp16
//     pieces like the direct kernel, three piece products per product on v_mfma_f32_32x32x16_f16, fp32 accumulate;
//   * weights are transformed on the host (G w, in double), scaled by a power of two, pre-split, stored as the MFMA B operand
//     [chunk][ky][position][piece][k-octet][co] x 16 B and streamed L2 -> VGPR two taps ahead;
//   * M = 32 tiles.  Tiles are numbered through the whole batch, row-pair-major ((crop, y/2), tx, y&1), so every M-tile is full
//     whatever S is (conv3: 100 tiles per crop = 3.125 M-tiles) and the 2x2 max-pool is a max over two accumulator registers of
//     one lane (rows y, y+1) and two of the four outputs of a tile; a pass = WM*TPW M-tiles, its real input rows (+2 halo
//     above / below, clipped at the crop: out-of-crop rows read a zero row) are contiguous in the batch's row numbering;
//   * 8 position accumulators per M-tile: TPW M-tiles per wave = TPW*128 accumulator registers, one wave per SIMD;
//   * output transform Y = A^T M, bias, ReLU, pool in the epilogue.
// LDS: [buffer][piece][row slot][position][tx][16 ci] fp16, slot 0 = zeros; double-buffered over the 16-channel chunks
// (the next chunk / next pass is transformed and stored in slices between the taps of the current one).
// ------------------------------------------------------------------------------------------------
// rows qmin .. qmin+nrows-1 (batch row numbering q = crop*S + y) that the tiles [T0, T0+MB) of a pass read
template <class G, int S>
__device__ __forceinline__ void wino_pass_rows(const int pass, const int total_tiles, int& qmin, int& nrows) {
    const int T0 = pass * G::MB;
    int TL = T0 + G::MB - 1;
    if (TL > total_tiles - 1) TL = total_tiles - 1;
    const int gp0 = T0 / G::TPP, gpl = TL / G::TPP;                     // first / last row pair (batch numbering)
    const int y0 = (2 * gp0) % S, yl = (2 * gpl) % S + 1;
    qmin = 2 * gp0 - (y0 >= 2 ? 2 : 0);
    const int qmax = 2 * gpl + 1 + (yl + 2 <= S - 1 ? 2 : 0);
    nrows = qmax - qmin + 1;
}

__device__ __forceinline__ uint32_t pack_h2(const _Float16 a, const _Float16 b) {
    return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
}

// raw buffer loads (SGPR resource + SGPR offset + 32-bit lane offset): no 64-bit address arithmetic on the VALU
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, const uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ uint4 buf_load16(const __amdgpu_buffer_rsrc_t r, const int voff, const int soff) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float4 buf_load16f(const __amdgpu_buffer_rsrc_t r, const int voff, const int soff) {
    // default cache policy: neighbouring tiles and neighbouring passes read the same pixels (x-overlap of the 8-pixel windows, y-halo),
    // and L2 has to absorb those re-reads -- with the nt hint every one of them went to HBM (8.4 GB per launch instead of ~4)
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// one fp32 value -> two fp16 pieces, round-toward-zero packing of two values at a time (v_cvt_pkrtz_f16_f32): the first piece may be
// any fp16 near x (the residual x - h1 is exact in fp32), the second loses at most one unit of the 22nd bit
typedef __fp16 h2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2h_pair(const float a, const float b, uint32_t& p1, uint32_t& p2) {
    const h2_t h1 = __builtin_amdgcn_cvt_pkrtz(a, b);
    // residuals a - h1.lo, b - h1.hi in one mixed-precision FMA each (the compiler's own choice is v_cvt_f32_f16 + v_sub_f32: twice the
    // instructions of a phase that runs at the vector rate); exact either way
    float ra, rb;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(h1), "v"(a));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(h1), "v"(b));
    const h2_t h2 = __builtin_amdgcn_cvt_pkrtz(ra, rb);
    p1 = __builtin_bit_cast(uint32_t, h1);
    p2 = __builtin_bit_cast(uint32_t, h2);
}

template <int CI, int CO, int S, int TPW>
__global__ __launch_bounds__((WinoGeom<CI, CO, S, TPW>::NTHR), (TPW == 1 ? 2 : 1)) void k_conv5_wino(const float* __restrict__ in /*[N][S][S][CI]*/,
                                                                               const uint4* __restrict__ wp /*[CI/16][5][8][2][2][CO] x 16 B*/,
                                                                               const float* __restrict__ bias, float* __restrict__ out,
                                                                               const float out_scale, uint32_t* __restrict__ overflow,
                                                                               const int n_crops, uint32_t* __restrict__ pass_ctr) {
    using G = WinoGeom<CI, CO, S, TPW>;
    static_assert(TPW == 1 || TPW == 2, "one or two M-tiles per wave");     // TPW = 1: 128 accumulator registers, two workgroups per CU
    extern __shared__ __attribute__((aligned(16))) uint8_t ldsb[];
    __shared__ int s_next_pass;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = wave % G::NT, mg = wave / G::NT;
    const int total_tiles = n_crops * G::TPC;
    const int n_pass = (total_tiles + G::MB - 1) / G::MB;
    int pass = blockIdx.x;
    if (pass >= n_pass) return;
    float mxabs = 0.f;                                   // largest |input| staged by this lane (fp16 range guard, see the end)

    // the zero row (slot 0) of both pieces of both buffers
    for (int i = tid; i < 4 * (G::RP / 16); i += G::NTHR) {
        const int pl = i / (G::RP / 16), o = i - pl * (G::RP / 16);
        *reinterpret_cast<uint4*>(ldsb + pl * G::PLANE + o * 16) = make_uint4(0, 0, 0, 0);
    }

    // Staging, branch-free so that it can sit between the MFMAs of the taps: one item = one tile (8 input pixels) x 4 input channels
    // of one row.  Rows past the pass's last row repeat that row (same bytes to the same place), columns outside the crop are
    // loaded from the clamped column and zeroed.  Steps of an item: L (8 x 16-byte loads), T (B^T of one channel), S (split two
    // positions of two channels into fp16 pieces, one 4-byte store per piece and position).
    float4 sdb[2][8];                                   // two items in flight: both are loaded at the head of a chunk, long before their use
    float su[2][8];
    int sdstb[2] = {0, 0}, sflagb[2] = {0, 0};
    __amdgpu_buffer_rsrc_t srs = make_rsrc(in, 0);
    // L: the eight loads of item item_ into buffer item_
#define WS_L(item_, cc_, qmin_, nrows_)                                                                                         \
    do {                                                                                                                        \
        const int idx_ = tid + (item_) * G::NTHR;                                                                               \
        int s_ = idx_ / (G::TPR * 4);                                                                                           \
        const int r_ = idx_ - s_ * (G::TPR * 4);                                                                                \
        const int cq_ = r_ & 3, tx_ = r_ >> 2;                                                                                  \
        s_ = s_ < (nrows_) ? s_ : (nrows_) - 1;                                                                                 \
        srs = make_rsrc(in + ((size_t)(qmin_) * S) * CI, (uint32_t)(G::NR * S * CI * 4));                                      \
        const int soff_ = s_ * (S * CI * 4) + (cc_) * 64 + cq_ * 16;                                                            \
        sdstb[item_] = (s_ + 1) * G::RP + tx_ * 32 + cq_ * 8;                                                                   \
        sflagb[item_] = (tx_ == 0 ? 1 : 0) | (tx_ == G::TPR - 1 ? 2 : 0);                                                       \
        _Pragma("unroll") for (int k_ = 0; k_ < 8; ++k_) {                                                                      \
            int ix_ = 4 * tx_ - 2 + k_;                                                                                         \
            ix_ = ix_ < 0 ? 0 : (ix_ > S - 1 ? S - 1 : ix_);                                                                    \
            sdb[item_][k_] = buf_load16f(srs, soff_ + ix_ * (CI * 4), 0);                                                    \
        }                                                                                                                       \
    } while (0)
    // T: B^T of one channel in two halves (positions 0, 7, 1, 2 then 3..6); the range guard rides on the first half
#define WS_T(item_, which_, comp_, hf_)                                                                                         \
    do {                                                                                                                        \
        const int sflag = sflagb[item_];                                                                                        \
        const float4* sd = sdb[item_];                                                                                          \
        const float d1_ = (sflag & 1) ? 0.f : sd[1].comp_, d6_ = (sflag & 2) ? 0.f : sd[6].comp_;                               \
        const float d2_ = sd[2].comp_, d3_ = sd[3].comp_, d4_ = sd[4].comp_, d5_ = sd[5].comp_;                                 \
        if ((hf_) == 0) {                                                                                                       \
            const float d0_ = (sflag & 1) ? 0.f : sd[0].comp_, d7_ = (sflag & 2) ? 0.f : sd[7].comp_;                           \
            mxabs = fmaxf(fmaxf(mxabs, fabsf(d2_)), fmaxf(fabsf(d3_), fmaxf(fabsf(d4_), fabsf(d5_))));                          \
            mxabs = fmaxf(fmaxf(mxabs, fabsf(d0_)), fmaxf(fabsf(d1_), fmaxf(fabsf(d6_), fabsf(d7_))));                          \
            su[which_][0] = fmaf(5.25f, d2_ - d4_, d6_ - d0_);                                                                  \
            su[which_][7] = fmaf(5.25f, d3_ - d5_, d7_ - d1_);                                                                  \
            const float e1_ = fmaf(-4.25f, d4_, d2_ + d6_), o1_ = fmaf(-4.25f, d3_, d1_ + d5_);                                 \
            su[which_][1] = e1_ + o1_; su[which_][2] = e1_ - o1_;                                                               \
        } else {                                                                                                                \
            const float e2_ = fmaf(-1.25f, d4_, fmaf(0.25f, d2_, d6_)), o2_ = fmaf(2.f, d5_, fmaf(-2.5f, d3_, 0.5f * d1_));     \
            su[which_][3] = e2_ + o2_; su[which_][4] = e2_ - o2_;                                                               \
            const float e3_ = fmaf(-5.f, d4_, fmaf(4.f, d2_, d6_)), o3_ = fmaf(0.5f, d5_, fmaf(-2.5f, d3_, 2.f * d1_));         \
            su[which_][5] = e3_ + o3_; su[which_][6] = e3_ - o3_;                                                               \
        }                                                                                                                       \
    } while (0)
    // S: four positions (4*pq_ .. 4*pq_+3) of two channels -> fp16 pieces, one 4-byte store per piece and position
#define WS_S(item_, pq_, half_, base_)                                                                                          \
    do {                                                                                                                        \
        _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) {                                                                      \
            uint32_t a1_, a2_;                                                                                                  \
            split2h_pair(su[0][4 * (pq_) + q_], su[1][4 * (pq_) + q_], a1_, a2_);                                               \
            uint8_t* dst_ = (base_) + sdstb[item_] + (4 * (pq_) + q_) * G::PS + (half_) * 4;                                    \
            *reinterpret_cast<uint32_t*>(dst_) = a1_;                                                                           \
            *reinterpret_cast<uint32_t*>(dst_ + G::PLANE) = a2_;                                                                \
        }                                                                                                                       \
    } while (0)
    // the 12 compute slots of one item: transform x, y (4) | stores (2) | transform z, w (4) | stores (2)
#define WS_STEP(st_, item_, base_)                                                                                              \
    do {                                                                                                                        \
        if ((st_) == 0) WS_T(item_, 0, x, 0);                                                                                   \
        if ((st_) == 1) WS_T(item_, 0, x, 1);                                                                                   \
        if ((st_) == 2) WS_T(item_, 1, y, 0);                                                                                   \
        if ((st_) == 3) WS_T(item_, 1, y, 1);                                                                                   \
        if ((st_) == 4) WS_S(item_, 0, 0, base_);                                                                               \
        if ((st_) == 5) WS_S(item_, 1, 0, base_);                                                                               \
        if ((st_) == 6) WS_T(item_, 0, z, 0);                                                                                   \
        if ((st_) == 7) WS_T(item_, 0, z, 1);                                                                                   \
        if ((st_) == 8) WS_T(item_, 1, w, 0);                                                                                   \
        if ((st_) == 9) WS_T(item_, 1, w, 1);                                                                                   \
        if ((st_) == 10) WS_S(item_, 0, 1, base_);                                                                              \
        if ((st_) == 11) WS_S(item_, 1, 1, base_);                                                                              \
    } while (0)
    constexpr int NIT = (G::NR * G::TPR * 4 + G::NTHR - 1) / G::NTHR;     // items per thread and chunk
    static_assert(NIT == 2, "two staging items per thread and chunk, 20 taps each");

    const __amdgpu_buffer_rsrc_t wrs = make_rsrc(wp, (uint32_t)(G::NCH * 40 * G::BV * 16));   // weights: SGPR resource + SGPR tap offset + lane offset
    const int boff = (h * CO + n * 32 + j) * 16;
    const int co = n * 32 + j;
    const float bz = bias[co];
    int qmin, nrows;
    wino_pass_rows<G, S>(pass, total_tiles, qmin, nrows);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {                                     // first pass: its first chunk
        WS_L(it, 0, qmin, nrows);
#pragma unroll
        for (int st = 0; st < 12; ++st) WS_STEP(st, it, ldsb);
    }
    __syncthreads();
    constexpr int BD = 3;                               // weight fragments are loaded BD taps ahead (L2 / MALL latency under load)
    uint4 bq[8][2];                                     // ring of 8: 40 taps per chunk keep the phase
#pragma unroll
    for (int t = 0; t < BD; ++t) {
        bq[t][0] = buf_load16(wrs, boff, t * G::BV * 16);
        bq[t][1] = buf_load16(wrs, boff, t * G::BV * 16 + 2 * CO * 16);
    }
    int bufsel = 0;
    for (;;) {
        // A-operand byte offsets of this lane's two tiles, one per kernel row (out-of-crop rows -> the zero row)
        int aoff[TPW][5];
        const int T0 = pass * G::MB + mg * TPW * 32;
#pragma unroll
        for (int m = 0; m < TPW; ++m) {
            int T = T0 + m * 32 + j;
            if (T > total_tiles - 1) T = total_tiles - 1;
            const int gp = T / G::TPP, r2 = T - gp * G::TPP;
            const int tx = r2 >> 1, qo = 2 * gp + (r2 & 1), y = qo % S;
#pragma unroll
            for (int ky = 0; ky < 5; ++ky) {
                const int iy = y + ky - 2;
                aoff[m][ky] = ((iy >= 0 && iy < S) ? (qo + ky - 2 - qmin + 1) * G::RP : 0) + tx * 32 + h * 16;
            }
        }
        f32x16 acc[TPW][8];
#pragma unroll
        for (int m = 0; m < TPW; ++m)
#pragma unroll
            for (int p = 0; p < 8; ++p)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][p][r] = 0.f;

        int next_pass = pass + (int)gridDim.x;
        if (tid == 0) s_next_pass = (int)atomicAdd(pass_ctr, 1u) + (int)gridDim.x;   // read by everyone after the first chunk's barrier
        bool have_next = false;
        int qmin_n = qmin, nrows_n = nrows;
        for (int cc = 0; cc < G::NCH; ++cc) {
            const bool last_c = cc == G::NCH - 1;
            if (last_c) {
                if (G::NCH == 1) __syncthreads();
                next_pass = s_next_pass;
                have_next = next_pass < n_pass;
                if (have_next) wino_pass_rows<G, S>(next_pass, total_tiles, qmin_n, nrows_n);
            }
            const uint8_t* pbase = ldsb + bufsel * G::BUF;
            uint8_t* nbase = ldsb + (bufsel ^ 1) * G::BUF;
            // what is staged under this chunk: the next chunk of this pass, or the first chunk of the next pass (without one: this
            // pass's first chunk once more, into the buffer nobody reads again -- cheaper than a branch around every slice)
            const int scc = last_c ? 0 : cc + 1;
            const int sqmin = last_c ? qmin_n : qmin, snrows = last_c ? nrows_n : nrows;
            const int wc = cc * 40 * G::BV * 16, wn = scc * 40 * G::BV * 16;
            uint4 af[2][TPW][2];
#pragma unroll
            for (int m = 0; m < TPW; ++m) {
                af[0][m][0] = *reinterpret_cast<const uint4*>(pbase + aoff[m][0]);
                af[0][m][1] = *reinterpret_cast<const uint4*>(pbase + aoff[m][0] + G::PLANE);
            }
#pragma clang loop unroll(full)
            for (int t = 0; t < 40; ++t) {
                const int cur = t & 1, nxt = cur ^ 1;
                if (t + 1 < 40) {                                    // A fragments of the next tap
                    const uint8_t* an = pbase + ((t + 1) % 8) * G::PS;
#pragma unroll
                    for (int m = 0; m < TPW; ++m) {
                        af[nxt][m][0] = *reinterpret_cast<const uint4*>(an + aoff[m][(t + 1) / 8]);
                        af[nxt][m][1] = *reinterpret_cast<const uint4*>(an + aoff[m][(t + 1) / 8] + G::PLANE);
                    }
                }
                const int wt = t + BD < 40 ? wc + (t + BD) * G::BV * 16 : wn + (t + BD - 40) * G::BV * 16;      // B fragments BD taps ahead
                bq[(t + BD) % 8][0] = buf_load16(wrs, boff, wt);
                bq[(t + BD) % 8][1] = buf_load16(wrs, boff, wt + 2 * CO * 16);
                // staging: item 0 loads at tap 0, slots 6..17; item 1 loads at tap 20, slots 26..37
                if (t == 0) WS_L(0, scc, sqmin, snrows);
                if (t == 20) WS_L(1, scc, sqmin, snrows);
                if (t >= 6 && t < 18) WS_STEP(t - 6, 0, nbase);
                if (t >= 26 && t < 38) WS_STEP(t - 26, 1, nbase);
                const int p = t % 8;
                const f16x8 b1 = __builtin_bit_cast(f16x8, bq[t % 8][0]);
                const f16x8 b2 = __builtin_bit_cast(f16x8, bq[t % 8][1]);
                f16x8 a1[TPW], a2[TPW];
#pragma unroll
                for (int m = 0; m < TPW; ++m) { a1[m] = __builtin_bit_cast(f16x8, af[cur][m][0]); a2[m] = __builtin_bit_cast(f16x8, af[cur][m][1]); }
#pragma unroll
                for (int m = 0; m < TPW; ++m) acc[m][p] = mfma16(a2[m], b1, acc[m][p]);
#pragma unroll
                for (int m = 0; m < TPW; ++m) acc[m][p] = mfma16(a1[m], b2, acc[m][p]);
#pragma unroll
                for (int m = 0; m < TPW; ++m) acc[m][p] = mfma16(a1[m], b1, acc[m][p]);
                // issue order inside a tap: next tap's A reads and the weight loads first (their latency hides under this tap's
                // MFMAs), then the MFMAs with the staging slice spread between them
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * TPW, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 10, 0);
#pragma unroll
                for (int g = 0; g < 3 * TPW; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x206, TPW == 1 ? 16 : 8, 0);
                }
                __builtin_amdgcn_sched_barrier(0);                  // keep the taps apart
            }
            __syncthreads();
            bufsel ^= 1;
        }
        // epilogue: Y = A^T M per tile (16-wide, one M-tile at a time: the four outputs of all 16 accumulator rows of a lane), then the
        // max over the 2x2 pool window (rows y, y+1 = registers r, r+1; outputs 0,1 / 2,3), bias, ReLU
#pragma unroll
        for (int m = 0; m < TPW; ++m) {
            f32x16 y0, y1, y2, y3;
            {
                const f32x16 e1 = acc[m][1] + acc[m][2], o1 = acc[m][1] - acc[m][2];
                y0 = acc[m][0] + e1; y1 = o1; y2 = e1; y3 = o1 + acc[m][7];
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                const f32x16 e2 = acc[m][3] + acc[m][4], o2 = acc[m][3] - acc[m][4];
                y0 += e2; y1 += 2.f * o2; y2 += 4.f * e2; y3 += 8.f * o2;
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                const f32x16 e3 = acc[m][5] + acc[m][6], o3 = acc[m][5] - acc[m][6];
                y0 += e3; y1 += 0.5f * o3; y2 += 0.25f * e3; y3 += 0.125f * o3;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const int r = 2 * rr;
                const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int T = T0 + m * 32 + i;
                const float v0 = fmaxf(fmaxf(y0[r], y1[r]), fmaxf(y0[r + 1], y1[r + 1]));
                const float v1 = fmaxf(fmaxf(y2[r], y3[r]), fmaxf(y2[r + 1], y3[r + 1]));
                if (T < total_tiles) {
                    const int gp = T / G::TPP, tx = (T - gp * G::TPP) >> 1;
                    float* o = out + ((size_t)gp * (S / 2) + 2 * tx) * CO + co;
                    __builtin_nontemporal_store(fmaxf(v0 * out_scale + bz, 0.f), o);
                    __builtin_nontemporal_store(fmaxf(v1 * out_scale + bz, 0.f), o + CO);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!have_next) break;
        pass = next_pass; qmin = qmin_n; nrows = nrows_n;
    }
#undef WS_L
#undef WS_T
#undef WS_S
#undef WS_STEP
    // fp16 range guard: |B^T d| <= 15 max|d| (largest absolute row sum of B^T), so inputs below 65520 / 15 cannot overflow a piece.
    // Larger (or non-finite) inputs raise the flag and the host-side guard re-runs the layer stack with the bf16 kernels.
    if (__any(!(mxabs < 4368.0f)) && lane == 0) atomicOr(overflow, 3u);
}

#include "cnn_wpre.h"
#include "cnn_conv3p.h"
#include "cnn_fused12.h"
#include "cnn_fused12rs.h"
#include "cnn_skip_kernels.h"

// ------------------------------------------------------------------------------------------------
// fc1: out[N][128] = act[N][K] * W[K][128] + b     (K = 12800, 100 real outputs)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fc1(const float* __restrict__ act, const float* __restrict__ w /*[K][128]*/,
                                             const float* __restrict__ bias /*[128]*/, float* __restrict__ out, int n, int K,
                                             const uint32_t* __restrict__ guard) {
    if (guard && guard[1] == 0u) return;                  // guard = the plan of k_guard_plan; list mode: row i of the GEMM is crop plan[2 + i]
    const int n_eff = fb_count(guard, n);
    if ((int)blockIdx.x * 32 >= n_eff) return;
    __shared__ float As[2][32 * 33];
    __shared__ __attribute__((aligned(16))) float Bs[2][32 * 128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * 32;
    // split-K: blockIdx.y takes K/gridDim.y consecutive inputs and writes its own partial plane (summed in k_head, fixed order)
    const int kspan = K / (int)gridDim.y, kbeg = (int)blockIdx.y * kspan;
    out += (size_t)blockIdx.y * n * 128;
    const int ar = tid >> 3, aq = tid & 7;                 // A tile: 32 rows x 8 float4
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float4 na, nb0, nb1, nb2, nb3;
    const bool arow = m0 + ar < n_eff;
    const float* asrc = act + (size_t)(arow ? plan_crop(guard, m0 + ar) : 0) * K + kbeg + aq * 4;
    const float4* wsrc = reinterpret_cast<const float4*>(w) + (size_t)kbeg * 32 + tid;
#define FC1_FETCH(k0)                                                                                  \
    do {                                                                                               \
        na = arow ? *reinterpret_cast<const float4*>(asrc + (k0)) : make_float4(0.f, 0.f, 0.f, 0.f);   \
        const float4* ws_ = wsrc + (size_t)(k0) * 32;                                                  \
        nb0 = ws_[0]; nb1 = ws_[256]; nb2 = ws_[512]; nb3 = ws_[768];                                  \
    } while (0)
#define FC1_STASH(buf)                                                                                 \
    do {                                                                                               \
        float* d_ = As[buf] + ar * 33 + aq * 4;                                                        \
        d_[0] = na.x; d_[1] = na.y; d_[2] = na.z; d_[3] = na.w;                                        \
        float4* b_ = reinterpret_cast<float4*>(Bs[buf]) + tid;                                         \
        b_[0] = nb0; b_[256] = nb1; b_[512] = nb2; b_[768] = nb3;                                      \
    } while (0)
    FC1_FETCH(0);
    FC1_STASH(0);
    __syncthreads();
    const int nk = kspan / 32;
    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nk) FC1_FETCH((kc + 1) * 32);          // next K chunk -> registers, overlaps the MFMAs below
        const float* as = As[buf] + j * 33 + h;
        const float* bs = Bs[buf] + h * 128 + wave * 32 + j;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[2 * t], bs[2 * t * 128], acc, 0, 0, 0);
        if (kc + 1 < nk) FC1_STASH(buf ^ 1);
        __syncthreads();
    }
#undef FC1_FETCH
#undef FC1_STASH
    const int co = wave * 32 + j;
    const float bz = blockIdx.y == 0 ? bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (m0 + i < n_eff) out[(size_t)plan_crop(guard, m0 + i) * 128 + co] = acc[r] + bz;
    }
}

// ------------------------------------------------------------------------------------------------
// fc1 on the fp16 matrix cores (default with the fp16 split convolutions): 128 crops x 128 outputs x 1/5 of K per block.
// Activations are split into two fp16 pieces while a 128 x 32 chunk is staged in LDS (80-byte row pitch: the 16 lanes of a
// ds_read_b128 group hit 16 distinct slots); weight fragments stream L2 -> VGPR from the pre-split image
// [k-octet][piece][co] x 8 halves.  3 MFMA products per product, fp32 accumulate; an activation outside the fp16 range
// raises the same flag as the convolutions (guarded fp32 re-run).
// ------------------------------------------------------------------------------------------------
// MT = tiles of 32 crops per workgroup.  4 (128 crops) for real batches; 1 for SMALL ones (TRex's default detect_batch_size of 1 gives 100 crops per
// call): ten workgroups walking 40 chunks of (load, split, barrier, 24 MFMAs) each took 54 us of a 234 us step -- a chain no prefetch depth shortens
// (four chunks in flight: 57 us); with 32 crops per workgroup the chain is a quarter as long per chunk and four times as many workgroups run it.
// Every output is the same sum in the same order whatever MT is.
// LISTED (cnn_skip3.h: skip3_fc1_listed): plane blockIdx.y computes only the crops of its list -- row r of the workgroup's tile is crop
// list[plane][m0 + r], the loads, the output rows and the crop flags go by that crop; rows behind the list's length load zeros and store
// nothing, whole 32-crop tiles behind it skip their MFMAs, a workgroup behind it returns at once.  A row's sum and its order are those of
// the dense form (a row of an MFMA tile depends on no other row); the head takes the planes that are not computed from Net::fc1e.
template <int MT = 4, bool LISTED = false>
__global__ __launch_bounds__(256) void k_fc1_split(const float* __restrict__ act, const uint4* __restrict__ wq /*[K/8][2][128]*/,
                                                   const float* __restrict__ bias, float* __restrict__ out, int n, int K,
                                                   const float out_scale, uint32_t* __restrict__ overflow, uint8_t* __restrict__ crop_flags,
                                                   const int* __restrict__ list /*[planes][stride]*/, const uint32_t* __restrict__ lens, const int stride) {
    constexpr int RPB = 80;                                     // bytes per staged row (32 halves + 16 pad)
    constexpr int RW = 32 * MT;                                 // crops per workgroup
    __shared__ __attribute__((aligned(16))) uint8_t As[2][2][RW * RPB];
    __shared__ int s_crop[LISTED ? RW : 1];                     // LISTED: the crop of every row of the tile (-1: behind the list)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * RW;
    const int len = LISTED ? (int)lens[blockIdx.y] : n;         // rows of this plane
    if (LISTED && m0 >= len) return;                            // (in front of every barrier)
    const int kspan = K / (int)gridDim.y, kbeg = (int)blockIdx.y * kspan;
    out += (size_t)blockIdx.y * n * 128;
    int crow[LISTED ? MT : 1];                                  // LISTED: the crop behind each row this thread stages
    if constexpr (LISTED) {
        list += (size_t)blockIdx.y * stride;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = (tid + 256 * i) >> 3;
            crow[i] = m0 + row < len ? list[m0 + row] : -1;
        }
        if (tid < RW) s_crop[tid] = m0 + tid < len ? list[m0 + tid] : -1;      // read behind the first barrier below
    }
    f32x16 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    bool ovf4[MT] = {};                // per staged row of this thread (row = crop): the range guard is per crop
    float4 na[MT];
    uint4 nb[2][2];
    const uint4* wl = wq + (size_t)(kbeg / 8) * 256 + wave * 32 + j;     // + (ko*2 + piece)*128
#define FCS_FETCH(kc)                                                                                                      \
    do {                                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                                                    \
            const int idx = tid + 256 * i, row = idx >> 3, q = idx & 7;                                                    \
            const int crop_ = LISTED ? crow[LISTED ? i : 0] : m0 + row < n ? m0 + row : -1;                                \
            na[i] = crop_ >= 0 ? *reinterpret_cast<const float4*>(act + (size_t)crop_ * K + kbeg + (kc) * 32 + q * 4)      \
                               : make_float4(0.f, 0.f, 0.f, 0.f);                                                          \
        }                                                                                                                  \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                                 \
            const uint4* w_ = wl + (size_t)((kc) * 4 + 2 * ks + h) * 256;                                                  \
            nb[ks][0] = w_[0]; nb[ks][1] = w_[128];                                                                        \
        }                                                                                                                  \
    } while (0)
#define FCS_STASH(buf)                                                                                                     \
    do {                                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                                                    \
            const int idx = tid + 256 * i, row = idx >> 3, q = idx & 7;                                                    \
            uint32_t a1[4], a2[4];                                                                                         \
            split2h(na[i].x, a1[0], a2[0], ovf4[i]); split2h(na[i].y, a1[1], a2[1], ovf4[i]);                              \
            split2h(na[i].z, a1[2], a2[2], ovf4[i]); split2h(na[i].w, a1[3], a2[3], ovf4[i]);                              \
            uint8_t* d = As[buf][0] + row * RPB + q * 8;                                                                   \
            *reinterpret_cast<uint2*>(d) = make_uint2(a1[0] | (a1[1] << 16), a1[2] | (a1[3] << 16));                       \
            *reinterpret_cast<uint2*>(d + RW * RPB) = make_uint2(a2[0] | (a2[1] << 16), a2[2] | (a2[3] << 16));           \
        }                                                                                                                  \
    } while (0)
    FCS_FETCH(0);
    FCS_STASH(0);
    uint4 cb[2][2] = {{nb[0][0], nb[0][1]}, {nb[1][0], nb[1][1]}};
    __syncthreads();
    const int nk = kspan / 32;
    for (int kc = 0; kc < nk; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nk) FCS_FETCH(kc + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const f16x8 b1 = __builtin_bit_cast(f16x8, cb[ks][0]), b2 = __builtin_bit_cast(f16x8, cb[ks][1]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (LISTED && m0 + 32 * m >= len) break;      // (uniform in the workgroup) a whole tile behind the list: nothing to add up
                const uint8_t* a = As[buf][0] + (32 * m + j) * RPB + (2 * ks + h) * 16;
                const f16x8 p1 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(a));
                const f16x8 p2 = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(a + RW * RPB));
                acc[m] = mfma16(p2, b1, acc[m]);
                acc[m] = mfma16(p1, b2, acc[m]);
                acc[m] = mfma16(p1, b1, acc[m]);
            }
        }
        if (kc + 1 < nk) {
            FCS_STASH(buf ^ 1);
            cb[0][0] = nb[0][0]; cb[0][1] = nb[0][1]; cb[1][0] = nb[1][0]; cb[1][1] = nb[1][1];
        }
        __syncthreads();
    }
#undef FCS_FETCH
#undef FCS_STASH
    bool any_ovf = false;
#pragma unroll
    for (int i = 0; i < MT; ++i) any_ovf |= ovf4[i];
    if (__any(any_ovf)) {
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const int row = (tid + 256 * i) >> 3;
            const int crop = LISTED ? crow[LISTED ? i : 0] : m0 + row < n ? m0 + row : -1;
            if (ovf4[i] && crop_flags && crop >= 0) crop_flags[crop] = 1;
        }
        if (lane == 0) atomicOr(overflow, 1u);
    }
    const int co = wave * 32 + j;
    const float bz = blockIdx.y == 0 ? bias[co] : 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int crop = LISTED ? s_crop[LISTED ? i : 0] : m0 + i < n ? m0 + i : -1;
            if (crop >= 0) out[(size_t)crop * 128 + co] = acc[m][r] * out_scale + bz;
        }
}

// ------------------------------------------------------------------------------------------------
// head: LayerNorm(100) + ReLU + fc2 + softmax, one wave per crop
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

// HEAD_CPW crops per wave: the fc2 weight of (input k, class c) is loaded once and serves the wave's crops (four independent sums per lane
// instead of one chain of 100 dependent loads + multiply-adds); per crop the operations and their order are those of one wave per crop
__global__ __launch_bounds__(256) void k_head(const float* __restrict__ fc1 /*[N][128]*/, const float* __restrict__ ln_g,
                                              const float* __restrict__ ln_b, const float* __restrict__ w2t /*[100][C]*/,
                                              const float* __restrict__ b2, float* __restrict__ probs /*[N][C]*/,
                                              float* __restrict__ logits_out, int n, int C, const uint32_t* __restrict__ guard, int ksplit,
                                              const float* __restrict__ fc1e /*[KSPLIT][128]*/, const int2* __restrict__ bands,
                                              const uint32_t* __restrict__ words) {
    // fc1e != nullptr: behind the listed fc1 (never with a guard: the re-run computes every plane of its crops) -- the plane of a pair that
    // is not listed (skip3_fc1_listed) was not computed: it is the empty crop's, the same bits
    if (guard && guard[1] == 0u) return;                   // guard = the plan of k_guard_plan; list mode: item i is crop plan[2 + i]
    const int n_items = fb_count(guard, n);
    constexpr int Q = HEAD_CPW;
    __shared__ float ys[4][Q][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int crop0 = (blockIdx.x * 4 + wave) * Q;
    if (crop0 >= n_items) return;
    const int nq = n_items - crop0 < Q ? n_items - crop0 : Q;            // crops of this wave (wave-uniform)
    int cidx[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) cidx[q] = plan_crop(guard, crop0 + (q < nq ? q : 0));
    const float g0 = ln_g[lane], be0 = ln_b[lane];
    const float g1 = lane + 64 < 100 ? ln_g[lane + 64] : 0.f, be1 = lane + 64 < 100 ? ln_b[lane + 64] : 0.f;
    // the fc1 partial planes of the split-K launch: every load of the wave's crops goes out first (the planes lie n * 512 bytes apart: a chain of
    // dependent loads would pay one memory latency per plane), the sums follow in the fixed plane order
    float xa[FC1_KSPLIT][Q], xb[FC1_KSPLIT][Q];
    const bool all = !fc1e || words[SK_EMPTY_RANGE] != 0;
    SkipBand band[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int2 b = all ? make_int2(0, 0) : bands[cidx[q]];
        band[q] = {b.x, b.y};
    }
#pragma unroll
    for (int s = 0; s < FC1_KSPLIT; ++s)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float* xs = skip3_fc1_listed(all, band[q], s) ? fc1 + (size_t)s * n * 128 + (size_t)cidx[q] * 128 : fc1e + s * 128;
            xa[s][q] = s < ksplit ? xs[lane] : 0.f;
            xb[s][q] = (s < ksplit && lane + 64 < 100) ? xs[lane + 64] : 0.f;
        }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (q >= nq) break;
        float x0 = xa[0][q], x1 = xb[0][q];
#pragma unroll
        for (int s = 1; s < FC1_KSPLIT; ++s)
            if (s < ksplit) { x0 += xa[s][q]; x1 += xb[s][q]; }
        const float mean = wave_sum(x0 + x1) * (1.f / 100.f);
        const float d0 = x0 - mean, d1 = lane + 64 < 100 ? x1 - mean : 0.f;
        const float var = wave_sum(d0 * d0 + d1 * d1) * (1.f / 100.f);     // biased variance (nn.LayerNorm)
        const float rstd = 1.f / sqrtf(var + 1e-5f);
        ys[wave][q][lane] = fmaxf(d0 * rstd * g0 + be0, 0.f);
        if (lane + 64 < 100) ys[wave][q][lane + 64] = fmaxf(d1 * rstd * g1 + be1, 0.f);
    }
    __builtin_amdgcn_wave_barrier();      // ys[wave] is private to this wave; LDS ops of one wave stay in order
    // logits: lane = class (stride 64), one 64-class slice at a time for all crops of the wave
    const int nrep = (C + 63) / 64;
    float mx[Q], sum[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) { mx[q] = -3.4e38f; sum[q] = 0.f; }
    float lg[16][Q];                      // up to 1024 classes (track_max_individuals default)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int q = 0; q < Q; ++q) lg[r][q] = -3.4e38f;
        if (r < nrep) {
            const int c = r * 64 + lane;
            if (c < C) {
                float s[Q];
                const float bias = b2[c];
#pragma unroll
                for (int q = 0; q < Q; ++q) s[q] = bias;
                for (int k = 0; k < 100; ++k) {
                    const float w = w2t[(size_t)k * C + c];
#pragma unroll
                    for (int q = 0; q < Q; ++q) s[q] = fmaf(ys[wave][q][k], w, s[q]);
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    lg[r][q] = s[q];
                    if (logits_out && q < nq) logits_out[(size_t)cidx[q] * C + c] = s[q];
                }
            }
#pragma unroll
            for (int q = 0; q < Q; ++q) mx[q] = fmaxf(mx[q], lg[r][q]);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) mx[q] = wave_max(mx[q]);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < nrep) {
            const int c = r * 64 + lane;
            if (c < C) {
#pragma unroll
                for (int q = 0; q < Q; ++q) { lg[r][q] = expf(lg[r][q] - mx[q]); sum[q] += lg[r][q]; }
            }
        }
#pragma unroll
    for (int q = 0; q < Q; ++q) sum[q] = 1.f / wave_sum(sum[q]);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < nrep) {
            const int c = r * 64 + lane;
            if (c < C) {
#pragma unroll
                for (int q = 0; q < Q; ++q) if (q < nq) probs[(size_t)cidx[q] * C + c] = lg[r][q] * sum[q];
            }
        }
}

// k_head for small batches (TRex's default detect_batch_size of 1: 100 crops per call).  k_head gives a wave four crops and walks fc2's 100
// inputs with one dependent global load per step: 25 us for 100 crops, all of it latency.  Here a wave has ONE crop (100 crops = 25 workgroups
// instead of 7), the LayerNorm outputs stay in registers and reach the lanes through v_readlane (no LDS), and the 100 weights of a class are
// fetched 25 at a time ahead of the multiply-adds.  The same operations in the same order per crop -- plane sums, LayerNorm, fc2 with the
// bias first and k ascending, softmax -- so the probabilities are bit-identical to k_head's (tests/test_cnn_gpu.py).
__global__ __launch_bounds__(256) void k_head_small(const float* __restrict__ fc1 /*[KSPLIT][N][128]*/, const float* __restrict__ ln_g,
                                                    const float* __restrict__ ln_b, const float* __restrict__ w2t /*[100][C]*/,
                                                    const float* __restrict__ b2, float* __restrict__ probs /*[N][C]*/,
                                                    float* __restrict__ logits_out, int n, int C, int ksplit,
                                                    uint32_t* __restrict__ overflow, uint8_t* __restrict__ crop_flags, uint32_t* __restrict__ plan) {
    // the re-run plan of the range guard (k_guard_plan's work: every kernel that can raise the flag lies in front of this one) by workgroup 0: one launch fewer
    __shared__ uint32_t plan_cnt;
    if (plan && blockIdx.x == 0) guard_plan<256>(overflow, crop_flags, n, plan, plan_cnt);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int crop = blockIdx.x * 4 + wave;
    if (crop >= n) return;
    const bool hi = lane + 64 < 100;
    float xa[FC1_KSPLIT], xb[FC1_KSPLIT];
#pragma unroll
    for (int s = 0; s < FC1_KSPLIT; ++s) {
        const float* xs = fc1 + (size_t)s * n * 128 + (size_t)crop * 128;
        xa[s] = s < ksplit ? xs[lane] : 0.f;
        xb[s] = (s < ksplit && hi) ? xs[lane + 64] : 0.f;
    }
    const float g0 = ln_g[lane], be0 = ln_b[lane];
    const float g1 = hi ? ln_g[lane + 64] : 0.f, be1 = hi ? ln_b[lane + 64] : 0.f;
    float x0 = xa[0], x1 = xb[0];
#pragma unroll
    for (int s = 1; s < FC1_KSPLIT; ++s)
        if (s < ksplit) { x0 += xa[s]; x1 += xb[s]; }
    const float mean = wave_sum(x0 + x1) * (1.f / 100.f);
    const float d0 = x0 - mean, d1 = hi ? x1 - mean : 0.f;
    const float var = wave_sum(d0 * d0 + d1 * d1) * (1.f / 100.f);
    const float rstd = 1.f / sqrtf(var + 1e-5f);
    const float y0 = fmaxf(d0 * rstd * g0 + be0, 0.f);            // input k of fc2 lives in lane k (k < 64) ...
    const float y1 = hi ? fmaxf(d1 * rstd * g1 + be1, 0.f) : 0.f; // ... or in lane k - 64
    const int nrep = (C + 63) / 64;
    float lg[16];
    float mx = -3.4e38f, sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        lg[r] = -3.4e38f;
        if (r < nrep) {
            const int c = r * 64 + lane;
            const int cc = c < C ? c : C - 1;                      // (every lane walks the loop: readlane wants the whole wave; the spare lanes repeat the last class)
            float s = b2[cc];
#pragma unroll
            for (int k0 = 0; k0 < 100; k0 += 25) {
                float w[25];
#pragma unroll
                for (int k = 0; k < 25; ++k) w[k] = w2t[(size_t)(k0 + k) * C + cc];
#pragma unroll
                for (int k = 0; k < 25; ++k) {
                    const int kk = k0 + k;
                    const float yk = kk < 64 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y0), kk))
                                             : __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y1), kk - 64));
                    s = fmaf(yk, w[k], s);
                }
            }
            if (c < C) {
                lg[r] = s;
                if (logits_out) logits_out[(size_t)crop * C + c] = s;
            }
            mx = fmaxf(mx, lg[r]);
        }
    }
    mx = wave_max(mx);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < nrep && r * 64 + lane < C) { lg[r] = expf(lg[r] - mx); sum += lg[r]; }
    sum = 1.f / wave_sum(sum);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < nrep && r * 64 + lane < C) probs[(size_t)crop * C + r * 64 + lane] = lg[r] * sum;
}

// ------------------------------------------------------------------------------------------------
// host: weight blob -> folded / repacked device tensors
// ------------------------------------------------------------------------------------------------
// an exec may still be running on its stream (launches are asynchronous): wait for the event recorded behind its last launch first
static void destroy_graph_entry(Net::GraphEntry& g) {
    if (g.exec) {
        if (g.last) (void)hipEventSynchronize(g.last);
        (void)hipGraphExecDestroy(g.exec);
    }
    if (g.last) (void)hipEventDestroy(g.last);
    g.exec = nullptr; g.last = nullptr;
}
static void drop_graphs(Net* n) {
    for (auto& g : n->graphs) destroy_graph_entry(g);
    n->graphs.clear();
}

void free_net(Net* n) {
    if (!n) return;
    drop_graphs(n);
    delete n->arch;
    n->weights.free_all();
    n->batch.free_all();
    delete n;
}

template <class T>
static int upload(Net* net, T** dst, const void* data, size_t bytes) {
    const int rc = net->weights.device_bytes(dst, bytes, "trexhip_load_weights");
    if (rc != TREXHIP_OK) return rc;
    TH_CHECK_HIP(hipMemcpy(*dst, data, bytes, hipMemcpyHostToDevice));
    return TREXHIP_OK;
}
template <class T, class V>
static int upload(Net* net, T** dst, const std::vector<V>& v) { return upload(net, dst, v.data(), v.size() * sizeof(V)); }
template <class T>
static int upload(Net* net, T** dst, float* inv, const ScaledImage& im) { *inv = im.inv; return upload(net, dst, im.v); }

#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)      // a chain of allocations stops at its first failure
static int make_empty_v3(trexhip_ctx* ctx, Net* net);
// parse -> pack (cnn_weights.hip) -> upload
int net_load(trexhip_ctx* ctx, const void* blob, size_t bytes) {
    ctx->prepared.weights_loaded();      // whatever was prepared was prepared for the network that goes
    const int arch = blob_arch_id(blob, bytes);
    if (arch >= TREXHIP_NET_V100 && arch <= TREXHIP_NET_V200) return arch_load(ctx, blob, bytes);      // the other architectures: cnn_arch.hip
    WeightBlob wb;
    const int prc = parse_weight_blob(blob, bytes, "trexhip_load_weights", &wb, [](int W, int H) -> int {
        if (W < 8 || W > 256 || H < 8 || H > 256) {
            set_error("trexhip_load_weights: individual_image_size " + std::to_string(W) + "x" + std::to_string(H) + " is outside 8..256 x 8..256");
            return TREXHIP_E_UNSUPPORTED;
        }
        return TREXHIP_OK;
    });
    if (prc != TREXHIP_OK) return prc;
    const int classes = wb.classes, W = wb.W, H = wb.H, CH = wb.CH;
    const bool at80 = W == 80 && H == 80;      // the tuned chain of this file; every other size runs the generic one of cnn_any.hip

    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    free_net(static_cast<Net*>(ctx->net));
    ctx->net = nullptr;
    Net* net = new Net();
    net->classes = classes; net->W = W; net->H = H; net->CH = CH;
    int rc = TREXHIP_OK;
    const Folded c1 = fold_conv1(&wb.t[T_C1W], CH);
    TRY(upload(net, &net->w1, c1.w)); TRY(upload(net, &net->b1, c1.b));
    if (at80) TRY(upload(net, &net->w1h, &net->inv1h, pack_conv1_frags(c1.w, CH)));
    const Folded c2 = fold_conv(&wb.t[T_C2W], 64, 16, 16);
    TRY(upload(net, &net->w2, c2.w)); TRY(upload(net, &net->b2, c2.b));
    TRY(upload(net, &net->w2s, pack_bf16x3(c2.w, 16, 64)));
    TRY(upload(net, &net->w2h, &net->inv2h, pack_f16x2(c2.w, 16, 64)));
    if (at80) TRY(upload(net, &net->w2w, &net->inv2w, pack_wino_f16(c2.w, 16, 64)));
    const Folded c3 = fold_conv(&wb.t[T_C3W], 128, 64, 16);           // 16-channel chunks for the matrix-core paths, 32 for exact fp32
    TRY(upload(net, &net->w3s, pack_bf16x3(c3.w, 64, 128)));
    TRY(upload(net, &net->w3h, &net->inv3h, pack_f16x2(c3.w, 64, 128)));
    if (at80) TRY(upload(net, &net->w3w, &net->inv3w, pack_wino_f16(c3.w, 64, 128)));
    TRY(net->weights.device_bytes(&net->d_ovf, OVF_WORDS * 4, "trexhip_load_weights"));
    if (rc == TREXHIP_OK && hipMemset(net->d_ovf, 0, OVF_WORDS * 4) != hipSuccess) rc = TREXHIP_E_DEVICE;
    const Folded c3x = fold_conv(&wb.t[T_C3W], 128, 64, 32);
    TRY(upload(net, &net->w3, c3x.w)); TRY(upload(net, &net->b3, c3x.b));
    const Folded f1 = pack_fc1(wb.t[T_F1W], wb.t[T_F1B], W, H);
    TRY(upload(net, &net->wf1, f1.w)); TRY(upload(net, &net->bf1, f1.b));
    if (at80) TRY(upload(net, &net->wf1h, &net->invf1h, pack_fc1_f16(f1.w)));          // (the generic chain's fc1 is exact fp32)
    TRY(upload(net, &net->lng, wb.t[T_LNG], 100 * sizeof(float)));
    TRY(upload(net, &net->lnb, wb.t[T_LNB], 100 * sizeof(float)));
    TRY(upload(net, &net->wf2t, pack_fc2(wb.t[T_F2W], classes)));
    TRY(upload(net, &net->bf2, wb.t[T_F2B], classes * sizeof(float)));
    if (at80 && CH == 1) TRY(make_empty_v3(ctx, net));
    if (rc != TREXHIP_OK) { free_net(net); return rc; }
    ctx->net = net;
    return TREXHIP_OK;
}

static int ensure_act(trexhip_ctx* ctx, Net* net, int n) {
    if (n <= net->max_crops) return TREXHIP_OK;
    drop_graphs(net);                                      // the captured chains point into the buffers that are replaced here
    ctx->prepared.batch_reallocated();                     // ... and so do the lists of a prepared call
    net->batch.free_all();
    net->h_probs = nullptr;
    net->max_crops = 0;
    Mem& B = net->batch;
    const char* who = "trexhip_identify_device";
    const size_t N = n;
    const size_t W = net->W, H = net->H;       // (80 x 80: 40 x 40 x 16, 20 x 20 x 64, 10 x 10 x 128)
    int rc = B.device_bytes(&net->d_ovfc, N, who);
    TRY(B.device_bytes(&net->act1, N * (H / 2) * (W / 2) * 16 * 4, who));
    TRY(B.device_bytes(&net->act2, N * (H / 4) * (W / 4) * 64 * 4, who));
    TRY(B.device_bytes(&net->act3, N * (H / 8) * (W / 8) * 128 * 4, who));
    TRY(B.device_bytes(&net->fc1, N * 128 * 4 * FC1_KSPLIT, who));
    TRY(B.device_bytes(&net->probs, N * net->classes * 4, who));
    TRY(B.device_bytes(&net->logits, N * net->classes * 4, who));
    if (W == 80 && H == 80) {                  // the Winograd-domain operand images of the 80 x 80 chain
        TRY(B.device_bytes(&net->v2, N * 40 * V2_ROWB, who));
        // (the empty crop's V3 image in front of V3 and behind it, in the same allocation: the listed conv3 reads background rows from the nearer
        // one through the buffer resource it reads V3 through, cnn_skip3.h)
        const size_t img = net->v3e ? (size_t)SkipGeom::V3_ROWS * V3_ROWB : 0;
        TRY(B.device_bytes(&net->v3, N * 20 * V3_ROWB + 2 * img, who));
        if (rc == TREXHIP_OK && img) {
            TH_CHECK_HIP(hipMemcpyAsync(net->v3, net->v3e, img, hipMemcpyDeviceToDevice, ctx->stream));
            TH_CHECK_HIP(hipMemcpyAsync(net->v3 + img + N * 20 * V3_ROWB, net->v3e, img, hipMemcpyDeviceToDevice, ctx->stream));
            net->v3 += img;
        }
    }
    if (net->v3e) {                            // the pass list of the role-split kernel
        const size_t n_pass = (N * SkipGeom::V3_ROWS + SkipGeom::RPP - 1) / SkipGeom::RPP;
        TRY(B.device_bytes(&net->skip_bands, N * sizeof(int2), who));
        TRY(B.device_bytes(&net->skip_counts, ((n_pass + SKIP_LB - 1) / SKIP_LB) * SKIP_NCNT * 4, who));
        TRY(B.device_bytes(&net->skip_list, (n_pass + SKIP_PAD) * 4, who));
        TRY(B.device_bytes(&net->skipx_cols, N * sizeof(int2), who));
        TRY(B.device_bytes(&net->skipx_list, (N * skipx_passes({0, SkipGeom::V3_ROWS - 1}) + SKIP_PAD) * 4, who));
        TRY(B.device_bytes(&net->skipx_rows, (N * skipx_passes({0, SkipGeom::V3_ROWS - 1}) + SKIP_PAD) * 4, who));
        const size_t blocks3 = (N + Skip3Geom::BLOCK - 1) / Skip3Geom::BLOCK;
        // (the lists of either form of a listed pass, pair slots or tile slots: the longer one)
        constexpr size_t BP3 = std::max(Skip3Geom::BLOCK_PASSES, Skip3TGeom::BLOCK_PASSES), BP3X = std::max(Skip3XGeom::BLOCK_PASSES, Skip3TXGeom::BLOCK_PASSES);
        static_assert(Skip3Geom::DESC == Skip3TGeom::DESC && Skip3XGeom::DESC == Skip3TXGeom::DESC, "one descriptor size per list");
        TRY(B.device_bytes(&net->skip3_counts, 2 * ((blocks3 + SKIP3_TB - 1) / SKIP3_TB) * sizeof(uint4), who));
        TRY(B.device_bytes(&net->skip3_tcounts, blocks3 * 2 * sizeof(uint32_t), who));
        TRY(B.device_bytes(&net->skip3_desc, blocks3 * BP3 * Skip3Geom::DESC * 4, who));
        TRY(B.device_bytes(&net->skip3_rows, blocks3 * BP3 * Skip3Reach::WORDS * 4, who));
        TRY(B.device_bytes(&net->skip3x_desc, blocks3 * BP3X * Skip3XGeom::DESC * 4, who));
        TRY(B.device_bytes(&net->skip3x_rows, blocks3 * BP3X * std::max(Skip3Reach::WORDS, Skip3TXGeom::ROW_WORDS) * 4, who));
        TRY(B.device_bytes(&net->fc1_list, Skip3Geom::PAIRS * N * sizeof(int), who));
    }
    TRY(B.device_bytes(&net->crops, N * net->W * net->H * net->CH, who));
    TRY(B.pinned(&net->h_probs, N * net->classes, who));
    if (rc != TREXHIP_OK) return rc;
    TH_CHECK_HIP(hipMemsetAsync(net->d_ovfc, 0, N, ctx->stream));      // on the stream its users run on; the plan kernel clears what it reads
    net->max_crops = n;
    return TREXHIP_OK;
}
#undef TRY

// ------------------------------------------------------------------------------------------------
// host: one forward pass = make the plan (cnn_plan.h), launch what it says, in order
// ------------------------------------------------------------------------------------------------
std::vector<LdsAttr>& lds_attrs() { static std::vector<LdsAttr> v; return v; }

// every kernel instance of this file's chains, once (the any-size convolutions: cnn_any.hip)
// (k_conv1's LDS depends on the channels alone at 80 x 80; it never had the attribute and is not listed for it)
static const ByChannels K_CONV1{Kern(k_conv1<1>, 256, (84 * 84 + 25 * 16) * 4, false), Kern(k_conv1<3>, 256, 3 * (84 * 84 + 25 * 16) * 4, false)};
static const ByChannels K_CONV1_MFMA{Kern(k_conv1_mfma, 256), Kern(k_conv1_mfma3, 256)};
static const ByChannels K_CONV1_WPRE{Kern(k_conv1_wpre<1>, 256), Kern(k_conv1_wpre<3>, 256)};
static const Kern K_CONV12_RS(k_conv12_rs<W12RGeom>, 512, W12RGeom::LDS_BYTES);
static const Kern K_CONV12_RSX(k_conv12_rs<W12XGeom>, 512, W12XGeom::LDS_BYTES);
static const Kern K_CONV12_WPRE(k_conv12_wpre, 256, W12Geom::LDS_BYTES);
static const Kern K_CROP_BANDS(k_crop_bands, 256);
static const Kern K_PASS_COUNT(k_pass_count, SKIP_LB);
static const Kern K_PASS_LIST(k_pass_list, SKIP_LB);
static const Kern K_V3_FILL(k_v3_fill, SKIP_FILL_TB);
static const Kern K_CONV2_WPRE2(k_conv2_wpre2, 256, W2bGeom::LDS_BYTES);
static const Kern K_CONV2_STREAM(k_conv5_stream<16, 64, 40, 8, 4>, 256, ConvGeomS<16, 64, 40, 8, 4>::LDS_BYTES);
using GW3 = WinoGeom<64, 128, 20, 2>;
static const Kern K_CONV3_WINO(k_conv5_wino<64, 128, 20, 2>, GW3::NTHR, GW3::LDS_BYTES);
static const Kern K_CONV3_WPAIR(k_conv5_wpair<false>, 256, GW3::LDS_BYTES + 1024 /* slack for the last DMA instruction */);
static const Kern K_CONV3_WPAIR_LIST(k_conv5_wpair<true>, 256, GW3::LDS_BYTES + 1024);
using GW3X = Wino3Pass<Skip3XGeom::TILES, Skip3XGeom::NR>;
static const Kern K_CONV3_WPAIR_LISTX(k_conv5_wpair<true, Skip3XGeom>, 256, GW3X::LDS_BYTES + 1024);
// (the listed instances on passes of tile slots, cnn_skip3.h, and the list kernels that make those)
using GW3T = Wino3Pass<Skip3TGeom::TILES, Skip3TGeom::NR>;
using GW3TX = Wino3Pass<Skip3TXGeom::TILES, Skip3TXGeom::NR>;
static const Kern K_CONV3_WPAIR_TLIST(k_conv5_wpair<true, Skip3TGeom>, 256, GW3T::LDS_BYTES + 1024);
static const Kern K_CONV3_WPAIR_TLISTX(k_conv5_wpair<true, Skip3TXGeom>, 256, GW3TX::LDS_BYTES + 1024);
static const Kern K_PAIR_COUNT(k_pair_count<false>, SKIP3_NT), K_PAIR_COUNT_T(k_pair_count<true>, SKIP3_NT_TILED);
static const Kern K_PAIR_LIST(k_pair_list<false>, SKIP3_NT), K_PAIR_LIST_T(k_pair_list<true>, SKIP3_NT);
static const Kern K_ACT3_FILL(k_act3_fill<false>, 256), K_ACT3_FILL_T(k_act3_fill<true>, 256);
template <int CI, int CO, int S, int ROWS, int NTERMS>
static auto split_kern() { return Kern(k_conv5_split<CI, CO, S, ROWS, NTERMS>, 512, ConvGeomB<CI, CO, S, ROWS, SPLIT_NP>::LDS_BYTES); }
// conv2 / conv3 on fp32 activations in the exact modes; x6_plan is the bf16x6 instance of every chain's guarded re-run
struct ExactLayer { decltype(Kern(k_conv5<16, 64, 40, 20, 16>, 512)) f32; decltype(split_kern<16, 64, 40, 10, 6>()) x6, x3, x6_plan; };
static const auto K_CONV2_X6 = split_kern<16, 64, 40, 10, 6>();
static const ExactLayer K_CONV2{Kern(k_conv5<16, 64, 40, 20, 16>, 512, ConvGeom<16, 64, 40, 20, 16>::LDS_BYTES), K_CONV2_X6, split_kern<16, 64, 40, 10, 3>(), K_CONV2_X6};
static const ExactLayer K_CONV3{Kern(k_conv5<64, 128, 20, 20, 32>, 512, ConvGeom<64, 128, 20, 20, 32>::LDS_BYTES), split_kern<64, 128, 20, 20, 6>(),
                                split_kern<64, 128, 20, 20, 3>(), split_kern<64, 128, 20, 4, 6>()};
static const Kern K_FC1(k_fc1, 256);
static const Kern K_FC1_SPLIT1(k_fc1_split<1>, 256), K_FC1_SPLIT4(k_fc1_split<4>, 256), K_FC1_SPLIT4_LIST(k_fc1_split<4, true>, 256);
static const Kern K_FC1_LIST(k_fc1_list, FC1L_TB);
static const Kern K_HEAD(k_head, 256);
static const Kern K_HEAD_SMALL(k_head_small, 256);
static const Kern K_GUARD_PLAN(k_guard_plan, 1024);

struct Pass {            // one forward pass: what every launch below needs
    const Net& net; const CnnPlan& p; hipStream_t s; int mode;
    const uint8_t* crops; int n; float *probs, *logits;
};

// a conv1 of its own, on every crop or (guard = the re-run plan) on the plan's
static void launch_conv1(const Pass& f, const Conv1 kind, const uint32_t* guard) {
    const Net& net = f.net;
    switch (kind) {
    case Conv1::FUSED: break;
    case Conv1::WPRE: K_CONV1_WPRE[net.CH](f.s, f.p.conv1_grid, f.crops, net.w1h, net.b1, net.v2, net.inv1h, net.ovf(OVF_RANGE)); break;
    case Conv1::MFMA: K_CONV1_MFMA[net.CH](f.s, f.p.conv1_grid, f.crops, net.w1h, net.b1, net.act1, net.inv1h, guard); break;
    case Conv1::VALU: K_CONV1[net.CH](f.s, f.p.conv1_grid, f.crops, net.w1, net.b1, net.act1, net.W); break;
    case Conv1::ANY: any_conv1(f.s, net, f.p, f.crops); break;
    }
}

// conv2 (layer 2) or conv3 on fp32 activations in an exact mode: FP32, BF16X6, BF16X3; with a guard the bf16x6 instance on the re-run plan
static void launch_exact(const Pass& f, const int layer, const int mode, const uint32_t* guard) {
    const Net& net = f.net;
    const bool c2 = layer == 2;
    const ExactLayer& K = c2 ? K_CONV2 : K_CONV3;
    const Launch& l = guard ? (c2 ? f.p.r_conv2 : f.p.r_conv3) : (c2 ? f.p.conv2 : f.p.conv3);
    const float *in = c2 ? net.act1 : net.act2, *b = c2 ? net.b2 : net.b3;
    float* out = c2 ? net.act2 : net.act3;
    if (mode == TREXHIP_CNN_FP32) K.f32(f.s, l.grid, in, c2 ? net.w2 : net.w3, b, out);
    else (guard ? K.x6_plan : mode == TREXHIP_CNN_BF16X6 ? K.x6 : K.x3)(f.s, l.grid, in, c2 ? net.w2s : net.w3s, b, out, 1.0f, guard, l.items);
}

// fc1 + head: either fc1 variant and either head on the whole batch, or (guard = the re-run plan) k_fc1 and k_head on the plan's crops
static void launch_tail(const Pass& f, const uint32_t* guard) {
    const Net& net = f.net;
    const CnnPlan& p = f.p;
    if (guard || p.fc1 == Fc1::EXACT)
        K_FC1(f.s, dim3(guard ? p.r_fc1_grid : p.fc1_grid, p.planes), net.act3, net.wf1, net.bf1, net.fc1, f.n, p.K, guard);
    else if (p.fc1_listed)      // only the listed (crop, plane) rows; the head takes the others from fc1e
        K_FC1_SPLIT4_LIST(f.s, dim3(p.fc1_grid, p.planes), net.act3, net.wf1h, net.bf1, net.fc1, f.n, p.K, net.invf1h, net.ovf(OVF_RANGE), net.d_ovfc,
                          net.fc1_list, net.d_skip + SK3_FC1_LEN, net.max_crops);
    else
        (p.fc1 == Fc1::SPLIT1 ? K_FC1_SPLIT1 : K_FC1_SPLIT4)(f.s, dim3(p.fc1_grid, p.planes), net.act3, net.wf1h, net.bf1, net.fc1, f.n, p.K, net.invf1h,
                                                            net.ovf(OVF_RANGE), net.d_ovfc, nullptr, nullptr, 0);
    if (guard || p.head == Head::BIG) {
        const bool listed = !guard && p.fc1_listed;
        K_HEAD(f.s, guard ? p.r_head_grid : p.head_grid, net.fc1, net.lng, net.lnb, net.wf2t, net.bf2, f.probs, f.logits, f.n, net.classes, guard, p.planes,
               listed ? net.fc1e : nullptr, listed ? net.skip_bands : nullptr, listed ? net.d_skip : nullptr);
    }
    else        // its first workgroup also makes the range guard's plan
        K_HEAD_SMALL(f.s, p.head_grid, net.fc1, net.lng, net.lnb, net.wf2t, net.bf2, f.probs, f.logits, f.n, net.classes, p.planes,
                     p.head_plans ? net.ovf(OVF_RANGE) : nullptr, net.d_ovfc, p.head_plans ? net.ovf(OVF_PLAN) : nullptr);
}

// the guarded re-run behind an FP16X3 pass, in bf16x6 on the plan
static void launch_rerun(const Pass& f) {
    const uint32_t* g = f.net.ovf(OVF_PLAN);
    if (!f.p.head_plans) K_GUARD_PLAN(f.s, 1, f.net.ovf(OVF_RANGE), f.net.d_ovfc, f.n, f.net.ovf(OVF_PLAN));
    if (f.p.rerun_conv1) launch_conv1(f, Conv1::MFMA, g);
    for (const int layer : {2, 3}) {
        if (f.p.chain == Chain::ANY_SIZE) any_conv(f.s, f.net, f.p, layer, TREXHIP_CNN_BF16X6, g);
        else launch_exact(f, layer, TREXHIP_CNN_BF16X6, g);
    }
    launch_tail(f, g);
}

// The V3 image of an all-zero crop, once per loaded network: k_conv12_rs itself on one zero crop, every pass computed, its own range-flag word.
// A net whose background activations leave the fp16 range raises that word, and the list kernels then list every pass (they read it on the device).
// Right behind it the act3 of that crop: the dense k_conv5_wpair itself on that image.
static int make_empty_v3(trexhip_ctx* ctx, Net* net) {
    const char* who = "trexhip_load_weights";
    uint8_t* zero = nullptr;
    int rc = net->weights.device_bytes(&net->v3e, (size_t)SkipGeom::V3_ROWS * V3_ROWB, who);
    if (rc == TREXHIP_OK) rc = net->weights.device_bytes(&net->act3e, (size_t)Skip3Geom::PAIRS * 10 * 128 * 4, who);
    if (rc == TREXHIP_OK) rc = net->weights.device_bytes(&net->fc1e, (size_t)FC1_KSPLIT * 128 * 4, who);
    if (rc == TREXHIP_OK) rc = net->weights.device_bytes(&net->d_skip, SK_WORDS * 4, who);
    if (rc == TREXHIP_OK) rc = net->weights.device_bytes(&net->act2e, (size_t)SkipGeom::V3_ROWS * 20 * 64 * 4, who);
    if (rc == TREXHIP_OK) rc = net->weights.device_bytes(&net->bgtab, (size_t)W2xGeom::NBG * W2xGeom::BG_UNITS * sizeof(uint4), who);
    if (rc == TREXHIP_OK) rc = net->weights.device_bytes(&zero, SkipGeom::CROP_ROWS * 80, who);
    if (rc != TREXHIP_OK) return rc;
    const CnnPlan p = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, GEOM_ROLE_SPLIT | GEOM_NO_SKIP, 1, ctx->n_cus);
    TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(K_CONV12_RS.fn), hipFuncAttributeMaxDynamicSharedMemorySize, K_CONV12_RS.lds));
    TH_CHECK_HIP(hipMemsetAsync(net->d_skip, 0, SK_WORDS * 4, ctx->stream));
    TH_CHECK_HIP(hipMemsetAsync(zero, 0, SkipGeom::CROP_ROWS * 80, ctx->stream));
    K_CONV12_RS(ctx->stream, p.conv2.grid, zero, net->w1h, net->b1, net->inv1h, net->w2w, net->b2, net->v3e, net->inv2w, net->d_skip + SK_EMPTY_RANGE, 1,
                net->d_skip + SK_EMPTY_CTR, p.pk2, nullptr, nullptr, nullptr, net->act2e, nullptr, nullptr);
    TH_CHECK_HIP(hipGetLastError());
    // the background row of the windowed instance, as each first tile sees it: that instance itself without a list, one workgroup (cnn_fused12rs.h)
    TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(K_CONV12_RSX.fn), hipFuncAttributeMaxDynamicSharedMemorySize, K_CONV12_RSX.lds));
    K_CONV12_RSX(ctx->stream, 1, zero, net->w1h, net->b1, net->inv1h, net->w2w, net->b2, net->v3e, net->inv2w, net->d_skip + SK_EMPTY_RANGE, 1,
                 net->d_skip + SKX_CTR, 1, nullptr, nullptr, nullptr, net->act2e, nullptr, net->bgtab);
    TH_CHECK_HIP(hipGetLastError());
    TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(K_CONV3_WPAIR.fn), hipFuncAttributeMaxDynamicSharedMemorySize, K_CONV3_WPAIR.lds));
    K_CONV3_WPAIR(ctx->stream, p.conv3.grid, net->v3e, net->w3w, net->b3, net->act3e, net->inv3w, 1, net->d_skip + SK3_EMPTY_CTR, p.n_big3, nullptr, nullptr, nullptr);
    TH_CHECK_HIP(hipGetLastError());
    // ... and that crop's fc1 planes: k_fc1_split<4> itself on that act3, one crop, every plane, its own range-flag word.  A background activation
    // outside the fp16 pieces' range raises the empty crop's flag: every pass and every pair is listed then, nothing is taken from these images
    const CnnPlan pf = cnn_plan(80, 80, 1, TREXHIP_CNN_FP16X3, true, 0, 1, ctx->n_cus);
    K_FC1_SPLIT4(ctx->stream, dim3(1, pf.planes), net->act3e, net->wf1h, net->bf1, net->fc1e, 1, pf.K, net->invf1h, net->d_skip + SK3_FC1E_RANGE, nullptr,
                 nullptr, nullptr, 0);
    TH_CHECK_HIP(hipGetLastError());
    uint32_t range = 0;
    TH_CHECK_HIP(hipMemcpyAsync(&range, net->d_skip + SK3_FC1E_RANGE, 4, hipMemcpyDeviceToHost, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (range) {
        const uint32_t one = 1;
        TH_CHECK_HIP(hipMemcpy(net->d_skip + SK_EMPTY_RANGE, &one, 4, hipMemcpyHostToDevice));
    }
    return TREXHIP_OK;
}

// The role-split chain's preparation (cnn_skip_kernels.h), in front of conv1+conv2: which passes, row pairs and fc1 rows the crops need, and the
// V3 rows of the others; every decision stays on the device.  `direct`: the listed conv3 reads background rows from the image, the fill copies
// only where the dense form runs
struct PrepArgs { long long alloc_rows; bool direct, x3 /* conv3's listed pairs in two lists, windowed passes and full-width ones */, tiled /* passes of tile slots */; };
static PrepArgs prep_args(const Net& net, const CnnPlan& p) {
    // the back image lies behind the ALLOCATION's rows, whatever this call's n is
    const long long alloc_rows = (long long)net.max_crops * SkipGeom::V3_ROWS;
    const bool direct = p.v3_direct && skip3_direct_fits(alloc_rows);
    return {alloc_rows, direct, p.skip3x && direct && skip3x_direct_fits(alloc_rows), p.skip3t && skip3t_direct_fits(alloc_rows)};
}
static void launch_skip_prep(const Pass& f, const bool direct, const bool x3, const bool tiled) {
    const Net& net = f.net;
    const CnnPlan& p = f.p;
    const int n = f.n, lb = ceil_div(p.conv2.items, SKIP_LB);
    int2* cols = p.skipx ? net.skipx_cols : nullptr;      // null: no crop gets a window, one list
    K_CROP_BANDS(f.s, ceil_div(n, 4), f.crops, n, net.skip_bands, cols || x3 ? net.skipx_cols : nullptr);
    K_PASS_COUNT(f.s, lb, net.skip_bands, cols, n, net.d_skip, net.skip_counts, (int)p.bgrows);
    K_PASS_LIST(f.s, lb, net.skip_bands, cols, n, net.d_skip, net.skip_counts, net.skip_list, net.skipx_list, net.skipx_rows, (int)p.bgrows);
    if (p.skip3) {     // the row pairs conv3 computes, packed into passes: the word that names its form tells the fill whether to copy
        // (skip3x: the crops with a window of conv3 tiles go into a list of their own; its column bands are the ones k_crop_bands writes for skipx)
        const int2* cols3 = x3 ? net.skipx_cols : nullptr;
        (tiled ? K_PAIR_COUNT_T : K_PAIR_COUNT)(f.s, p.skip3_grid, net.skip_bands, cols3, n, net.d_skip, net.skip3_counts, net.skip3_tcounts);
        (tiled ? K_PAIR_LIST_T : K_PAIR_LIST)(f.s, p.skip3_grid, net.skip_bands, cols3, n, net.d_skip, net.skip3_counts, net.skip3_tcounts, net.skip3_desc, net.skip3x_desc);
        // the crops each plane of the listed fc1 computes: from the bands alone, so here and not between conv3 and fc1
        if (p.fc1_listed) K_FC1_LIST(f.s, Skip3Geom::PAIRS, net.skip_bands, n, net.d_skip, net.fc1_list, net.max_crops);
    }
    K_V3_FILL(f.s, ceil_div(n * SkipGeom::V3_ROWS, SKIP_FILL_TB), net.skip_bands, cols, n, net.d_skip, reinterpret_cast<const uint4*>(net.v3e),
              reinterpret_cast<uint4*>(net.v3), (int)direct);
}

// The launches of a role-split pass that read nothing but the crops and the loaded network, stated once: PREP_LISTS in front of conv1+conv2,
// PREP_ACT3 -- the listed passes' descriptors and row sources, and the other pairs' act3 -- in front of conv3, or both at once ahead of the pass
// (trexhip_identify_prepare_device): k_act3_fill reads what the list kernels wrote and nothing of conv1+conv2's.  Which form of conv3 runs is the
// device's word
// (PREP_ACT3 alone is only ever launched behind the PREP_LISTS of the same pass: k_act3_fill turns the runs k_pair_list left in the descriptors
// into descriptors IN PLACE, so a second fill without a list pass in between would read descriptors as runs)
enum : int { PREP_LISTS = 1, PREP_ACT3 = 2 };
static bool plan_prepares(const CnnPlan& p) { return p.chain == Chain::ROLE_SPLIT && p.skip; }
static void launch_prep(const Pass& f, const int parts) {
    const Net& net = f.net;
    const CnnPlan& p = f.p;
    if (!plan_prepares(p)) return;
    const PrepArgs a = prep_args(net, p);
    if (parts & PREP_LISTS) launch_skip_prep(f, a.direct, a.x3, a.tiled);
    if ((parts & PREP_ACT3) && p.skip3)
        (a.tiled ? K_ACT3_FILL_T : K_ACT3_FILL)(f.s, p.act3_fill.grid, net.skip_bands, a.x3 ? net.skipx_cols : nullptr, f.n, net.d_skip, reinterpret_cast<const uint4*>(net.act3e),
                    reinterpret_cast<uint4*>(net.act3), net.skip3_desc, net.skip3_rows, net.skip3x_desc, net.skip3x_rows, a.alloc_rows, (int)a.direct, (int)!p.fc1_listed);
}

static int set_cnn_attrs(trexhip_ctx* ctx) {
    if (!ctx->attr_cnn) {
        for (const LdsAttr& a : lds_attrs()) TH_CHECK_HIP(hipFuncSetAttribute(a.fn, hipFuncAttributeMaxDynamicSharedMemorySize, a.bytes));
        ctx->attr_cnn = true;
    }
    return TREXHIP_OK;
}

// prepared: launch_prep(f, PREP_LISTS | PREP_ACT3) for this very pass is queued on the stream already (cnn_prepared.h)
static int net_forward_launch(trexhip_ctx* ctx, const uint8_t* d_crops, int n, float* d_probs, float* d_logits, const bool prepared = false) {
    const Net& net = *static_cast<Net*>(ctx->net);
    if (const int rc = set_cnn_attrs(ctx)) return rc;
    const CnnPlan p = cnn_plan(net.W, net.H, net.CH, ctx->cnn_mode, (reinterpret_cast<uintptr_t>(d_crops) & 15) == 0, ctx->tune_conv_geom, n, ctx->n_cus);
    const Pass f{net, p, ctx->stream, ctx->cnn_mode, d_crops, n, d_probs, d_logits};
    hipStream_t s = f.s;
    const bool x3 = prep_args(net, p).x3, tiled = prep_args(net, p).tiled;
    // (the guard words in front of the plan start at zero: the plan's writer -- the last reader of all three -- hands them back zeroed; net_forward
    // clears them itself behind a pass that was not queued to its end)
    stage_begin(ctx, TREXHIP_STAGE_CNN_ALL);
    launch_conv1(f, p.conv1, nullptr);
    if (p.chain == Chain::ANY_SIZE) {
        any_conv(s, net, p, 2, f.mode, nullptr);
        any_conv(s, net, p, 3, f.mode, nullptr);
    } else {
        const bool pre = p.chain == Chain::ROLE_SPLIT || p.chain == Chain::FUSED_2WG || p.chain == Chain::TWO_KERNEL;      // conv2 writes V3
        stage_begin(ctx, TREXHIP_STAGE_CONV2);
        switch (p.chain) {
        case Chain::ROLE_SPLIT:
            if (!prepared) launch_prep(f, PREP_LISTS);
            // (an instance whose list is empty returns at once)
            if (p.skipx)
                K_CONV12_RSX(s, p.conv2.grid, d_crops, net.w1h, net.b1, net.inv1h, net.w2w, net.b2, net.v3, net.inv2w, net.ovf(OVF_RANGE), n, net.d_skip + SKX_CTR,
                             p.pk2, net.d_ovfc, net.skipx_list, net.d_skip + SKX_PASSES, net.act2e, net.skipx_rows, net.bgtab);
            K_CONV12_RS(s, p.conv2.grid, d_crops, net.w1h, net.b1, net.inv1h, net.w2w, net.b2, net.v3, net.inv2w, net.ovf(OVF_RANGE), n, net.ovf(OVF_PASS2),
                        p.pk2, net.d_ovfc, p.skip ? net.skip_list : nullptr, p.skip ? net.d_skip + (p.skipx ? SKX_FULL : SK_LEN) : nullptr, nullptr, nullptr, nullptr);
            break;
        case Chain::FUSED_2WG:
            K_CONV12_WPRE(s, p.conv2.grid, d_crops, net.w1h, net.b1, net.inv1h, net.w2w, net.b2, net.v3, net.inv2w, net.ovf(OVF_RANGE), n, net.ovf(OVF_PASS2),
                          p.pk2, net.d_ovfc);
            break;
        case Chain::TWO_KERNEL:
            K_CONV2_WPRE2(s, p.conv2.grid, net.v2, net.w2w, net.b2, net.v3, net.inv2w, net.ovf(OVF_RANGE), n, net.ovf(OVF_PASS2));
            break;
        case Chain::FP32_ACT:
            K_CONV2_STREAM(s, p.conv2.grid, net.act1, net.w2h, net.b2, net.act2, net.inv2h, net.ovf(OVF_RANGE), p.conv2.items);
            break;
        default: launch_exact(f, 2, f.mode, nullptr);
        }
        stage_end(ctx, TREXHIP_STAGE_CONV2);
        stage_begin(ctx, TREXHIP_STAGE_CONV3);
        if (pre) {
            if (p.skip3) {
                if (!prepared) launch_prep(f, PREP_ACT3);
                // (an instance whose list is empty returns at once)
                if (x3)
                    (tiled ? K_CONV3_WPAIR_TLISTX : K_CONV3_WPAIR_LISTX)(s, p.conv3.grid, net.v3, net.w3w, net.b3, net.act3, net.inv3w, n, net.d_skip + SK3X_CTR, 0, net.skip3x_desc, net.skip3x_rows, net.d_skip);
                (tiled ? K_CONV3_WPAIR_TLIST : K_CONV3_WPAIR_LIST)(s, p.conv3.grid, net.v3, net.w3w, net.b3, net.act3, net.inv3w, n, net.ovf(OVF_PASS3), 0, net.skip3_desc, net.skip3_rows, net.d_skip);
            }
            K_CONV3_WPAIR(s, p.conv3.grid, net.v3, net.w3w, net.b3, net.act3, net.inv3w, n, net.ovf(OVF_PASS3), p.n_big3, nullptr, nullptr, p.skip3 ? net.d_skip : nullptr);
        }
        else if (p.chain == Chain::FP32_ACT)
            K_CONV3_WINO(s, p.conv3.grid, net.act2, net.w3w, net.b3, net.act3, net.inv3w, net.ovf(OVF_RANGE), n, net.ovf(OVF_PASS3));
        else launch_exact(f, 3, f.mode, nullptr);
        stage_end(ctx, TREXHIP_STAGE_CONV3);
    }
    launch_tail(f, nullptr);
    if (p.rerun) launch_rerun(f);
    stage_end(ctx, TREXHIP_STAGE_CNN_ALL);
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

static constexpr int GRAPH_MAX_CROPS = 6400;      // above this the kernels themselves dominate
static constexpr size_t GRAPH_CACHE = 8;
static constexpr int GRAPH_MIN_SEEN = 3;          // calls with the same key before its chain is captured

// a call's chain is counted, captured or replayed (net_forward_inner) -- not launched as it stands
static bool graph_path(const trexhip_ctx* ctx, const Net* net, const int n) {
    static const bool enabled = [] { const char* e = std::getenv("TREXHIP_GRAPHS"); return !(e && std::atoi(e) == 0); }();
    // not while profiling (the stage events are host-side bookkeeping), not before the first plain call (function attributes are set there)
    return enabled && net->graphs_ok && n <= GRAPH_MAX_CROPS && !ctx->profiling && ctx->attr_cnn;
}

static int net_forward_inner(trexhip_ctx* ctx, const uint8_t* d_crops, int n, float* d_probs, float* d_logits, bool prepared);
int net_forward(trexhip_ctx* ctx, const uint8_t* d_crops, int n, float* d_probs, float* d_logits) {
    Net* net = static_cast<Net*>(ctx->net);
    // every forward pass takes the record of a prepare call; only the pass it was made for finds its launches done (cnn_prepared.h)
    const bool prepared = ctx->prepared.consume(ctx->prepared.make(d_crops, n, ctx->cnn_mode, ctx->tune_conv_geom, ctx->stream));
    if (ctx->cnn_mode == TREXHIP_CNN_FP16X3) {
        // the range flag and the pass counters: zero by construction (the plan kernel of the previous pass), cleared here only behind a pass that
        // failed half-way (outside any capture: a replayed chain never holds this memset)
        if (!net->ovf_clean) TH_CHECK_HIP(hipMemsetAsync(net->d_ovf, 0, OVF_PLAN * 4, ctx->stream));
        net->ovf_clean = false;
    }
    const int rc = net_forward_inner(ctx, d_crops, n, d_probs, d_logits, prepared);
    if (rc == TREXHIP_OK) { net->last_mode = ctx->cnn_mode; if (ctx->cnn_mode == TREXHIP_CNN_FP16X3) net->ovf_clean = true; }
    // (the plan is a pure function of these: the same one the launch, or the capture that is replayed, was made from)
    net->last_fc1_n = rc == TREXHIP_OK && !net->arch && cnn_plan(net->W, net->H, net->CH, ctx->cnn_mode, (reinterpret_cast<uintptr_t>(d_crops) & 15) == 0,
                                                                 ctx->tune_conv_geom, n, ctx->n_cus).fc1_listed ? n : 0;
    return rc;
}

// captures the chain of one call into `cand`; false (and graphs off for the net) when any step of that fails -- nothing was executed then
static bool capture_chain(trexhip_ctx* ctx, Net* net, Net::GraphEntry* cand, const uint8_t* d_crops, int n, float* d_probs, float* d_logits) {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipEvent_t ev = nullptr;
    bool ok = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        const int rc = net_forward_launch(ctx, d_crops, n, d_probs, d_logits);
        const hipError_t e_end = hipStreamEndCapture(ctx->stream, &graph);
        ok = rc == TREXHIP_OK && e_end == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess &&
             hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess;
    }
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) {
        (void)hipGetLastError();
        if (exec) (void)hipGraphExecDestroy(exec);
        net->graphs_ok = false;
        return false;
    }
    cand->exec = exec; cand->last = ev;
    return true;
}

static int net_forward_inner(trexhip_ctx* ctx, const uint8_t* d_crops, int n, float* d_probs, float* d_logits, const bool prepared) {
    Net* net = static_cast<Net*>(ctx->net);
    if (net->arch) return arch_forward(ctx, *net, d_crops, n, d_probs, d_logits);      // chunked, never captured
    // (a prepared call that ends up on the graph path -- the timers were switched off in between -- runs its whole chain)
    if (!graph_path(ctx, net, n)) return net_forward_launch(ctx, d_crops, n, d_probs, d_logits, prepared);
    hipStream_t s = ctx->stream;
    const Net::GraphKey key{d_crops, n, d_probs, d_logits, ctx->cnn_mode, ctx->tune_conv_geom, s};
    ++net->tick;
    Net::GraphEntry* cand = nullptr;
    for (auto& g : net->graphs)
        if (g.key == key) { cand = &g; break; }
    if (!cand) {                                                  // a new key: count it, run the chain directly
        if (net->graphs.size() >= GRAPH_CACHE) {                  // ... in the place of the least recently used one
            size_t lru = 0;
            for (size_t i = 1; i < net->graphs.size(); ++i) if (net->graphs[i].used < net->graphs[lru].used) lru = i;
            destroy_graph_entry(net->graphs[lru]);
            net->graphs.erase(net->graphs.begin() + (long)lru);
        }
        net->graphs.push_back({key, nullptr, net->tick, nullptr, 1});
        return net_forward_launch(ctx, d_crops, n, d_probs, d_logits);
    }
    cand->used = net->tick;
    if (!cand->exec && (++cand->seen < GRAPH_MIN_SEEN || !capture_chain(ctx, net, cand, d_crops, n, d_probs, d_logits)))
        return net_forward_launch(ctx, d_crops, n, d_probs, d_logits);
    TH_CHECK_HIP(hipGraphLaunch(cand->exec, s));
    TH_CHECK_HIP(hipEventRecord(cand->last, s));
    return TREXHIP_OK;
}

// the checks and preparations every identify entry point shares; *net stays null when there is nothing to do (n == 0)
static int identify_prepare(trexhip_ctx* ctx, const bool args, const char* who, const int32_t n, Net** net) {
    *net = nullptr;
    if (!args) { set_error(std::string(who) + ": null argument"); return TREXHIP_E_INVALID; }
    Net* loaded = static_cast<Net*>(ctx->net);
    if (!loaded) { set_error("trexhip_identify: weights not loaded (VINetwork status().weights.loaded())"); return TREXHIP_E_INVALID; }
    if (n < 0) { set_error("trexhip_identify: n < 0"); return TREXHIP_E_INVALID; }
    if (n == 0) return TREXHIP_OK;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    const int rc = loaded->arch ? arch_ensure_act(ctx, loaded, n) : ensure_act(ctx, loaded, n);
    if (rc == TREXHIP_OK) *net = loaded;
    return rc;
}

}  // namespace trexhip

using namespace trexhip;

extern "C" {

int trexhip_load_weights(trexhip_ctx* ctx, const void* blob, size_t bytes) {
    if (!ctx || !blob) { set_error("trexhip_load_weights: null argument"); return TREXHIP_E_INVALID; }
    return net_load(ctx, blob, bytes);
}

int trexhip_identify_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n, float* d_probs, float* d_logits) {
    Net* net;
    const int rc = identify_prepare(ctx, ctx && d_crops && d_probs, "trexhip_identify_device", n, &net);
    if (rc || !net) return rc;
    return net_forward(ctx, d_crops, n, d_probs, d_logits);
}

int trexhip_identify_prepare_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n) {
    Net* net;
    const int rc = identify_prepare(ctx, ctx && d_crops, "trexhip_identify_prepare_device", n, &net);
    if (rc || !net) return rc;
    ctx->prepared.drop();
    if (net->arch || ctx->cnn_mode != TREXHIP_CNN_FP16X3 || graph_path(ctx, net, n)) return TREXHIP_OK;
    const CnnPlan p = cnn_plan(net->W, net->H, net->CH, ctx->cnn_mode, (reinterpret_cast<uintptr_t>(d_crops) & 15) == 0, ctx->tune_conv_geom, n, ctx->n_cus);
    if (!plan_prepares(p)) return TREXHIP_OK;
    const Pass f{*net, p, ctx->stream, ctx->cnn_mode, d_crops, n, nullptr, nullptr};
    stage_begin(ctx, TREXHIP_STAGE_PREPARE);
    launch_prep(f, PREP_LISTS | PREP_ACT3);
    stage_end(ctx, TREXHIP_STAGE_PREPARE);
    TH_CHECK_HIP(hipGetLastError());
    ctx->prepared.set(ctx->prepared.make(d_crops, n, ctx->cnn_mode, ctx->tune_conv_geom, ctx->stream));
    return TREXHIP_OK;
}

int trexhip_identify_prepare_stats(trexhip_ctx* ctx, uint32_t* records, uint32_t* hits) {
    if (!ctx) { set_error("trexhip_identify_prepare_stats: null ctx"); return TREXHIP_E_INVALID; }
    if (records) *records = ctx->prepared.records;
    if (hits) *hits = ctx->prepared.hits;
    return TREXHIP_OK;
}

int trexhip_identify(trexhip_ctx* ctx, const uint8_t* crops, int32_t n, float* probs) {
    Net* net;
    int rc = identify_prepare(ctx, ctx && crops && probs, "trexhip_identify", n, &net);
    if (rc || !net) return rc;
    const size_t cb = (size_t)net->W * net->H * net->CH;
    TH_CHECK_HIP(hipMemcpyAsync(net->crops, crops, cb * n, hipMemcpyHostToDevice, ctx->stream));
    rc = net_forward(ctx, net->crops, n, net->probs, nullptr);
    if (rc) return rc;
    TH_CHECK_HIP(hipMemcpyAsync(probs, net->probs, (size_t)n * net->classes * 4, hipMemcpyDeviceToHost, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return TREXHIP_OK;
}

int trexhip_identify_guard_stats(trexhip_ctx* ctx, uint32_t* rerun_crops, uint32_t* whole_batch) {
    if (!ctx || !ctx->net) { set_error("trexhip_identify_guard_stats: no context / weights not loaded"); return TREXHIP_E_INVALID; }
    Net* net = static_cast<Net*>(ctx->net);
    uint32_t plan[2] = {0, 0};
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    // the plan of the LAST forward pass -- none before the first pass or behind a pass in another precision mode (not ctx->cnn_mode, which
    // trexhip_set_identity_precision may have changed since)
    if (net->last_mode == TREXHIP_CNN_FP16X3 && net->arch) {      // the chunks of the call together (k_arch_guard_plan)
        uint32_t st[2] = {0, 0};
        TH_CHECK_HIP(hipMemcpy(st, net->ovf(ARCH_STAT_RERUN), 8, hipMemcpyDeviceToHost));
        if (rerun_crops) *rerun_crops = st[0];
        if (whole_batch) *whole_batch = st[1] ? 1u : 0u;
        return TREXHIP_OK;
    }
    if (net->last_mode == TREXHIP_CNN_FP16X3) TH_CHECK_HIP(hipMemcpy(plan, net->ovf(OVF_PLAN), 8, hipMemcpyDeviceToHost));
    if (rerun_crops) *rerun_crops = plan[1] == 1u ? plan[0] : 0u;
    if (whole_batch) *whole_batch = plan[1] == 2u ? 1u : 0u;
    return TREXHIP_OK;
}

// the words of Net::d_skip as the queued work leaves them (zeros: a network without them)
static int read_skip_words(trexhip_ctx* ctx, const char* who, uint32_t (&w)[SK_WORDS]) {
    if (!ctx || !ctx->net) { set_error(std::string(who) + ": no context / weights not loaded"); return TREXHIP_E_INVALID; }
    const Net* net = static_cast<Net*>(ctx->net);
    std::fill(w, w + SK_WORDS, 0u);
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    if (net->d_skip) TH_CHECK_HIP(hipMemcpy(w, net->d_skip, sizeof w, hipMemcpyDeviceToHost));
    return TREXHIP_OK;
}

int trexhip_identify_skip_stats(trexhip_ctx* ctx, uint32_t* passes, uint32_t* listed, uint64_t* bytes_filled) {
    uint32_t w[SK_WORDS];
    if (const int rc = read_skip_words(ctx, "trexhip_identify_skip_stats", w)) return rc;
    if (passes) *passes = w[SK_NPASS];
    if (listed) *listed = w[SK_LEN];
    if (bytes_filled) *bytes_filled = (uint64_t)w[SK_FILLED] * V3_ROWB;
    return TREXHIP_OK;
}

int trexhip_identify_skipx_stats(trexhip_ctx* ctx, uint32_t* crops_windowed, uint32_t* windowed_passes, uint32_t* full_passes) {
    uint32_t w[SK_WORDS];
    if (const int rc = read_skip_words(ctx, "trexhip_identify_skipx_stats", w)) return rc;
    if (crops_windowed) *crops_windowed = w[SKX_CROPS];
    if (windowed_passes) *windowed_passes = w[SKX_PASSES];
    if (full_passes) *full_passes = w[SKX_FULL];
    return TREXHIP_OK;
}

int trexhip_identify_bgrow_stats(trexhip_ctx* ctx, uint32_t* rows_read, uint32_t* rows_made) {
    uint32_t w[SK_WORDS];
    if (const int rc = read_skip_words(ctx, "trexhip_identify_bgrow_stats", w)) return rc;
    if (rows_read) *rows_read = w[SKX_V2_READ];
    if (rows_made) *rows_made = w[SKX_V2_MADE];
    return TREXHIP_OK;
}

int trexhip_identify_skip3x_stats(trexhip_ctx* ctx, uint32_t* crops_windowed, uint32_t* windowed_passes, uint32_t* full_passes) {
    uint32_t w[SK_WORDS];
    if (const int rc = read_skip_words(ctx, "trexhip_identify_skip3x_stats", w)) return rc;
    if (crops_windowed) *crops_windowed = w[SK3_USE] ? w[SK3X_CROPS] : 0u;
    if (windowed_passes) *windowed_passes = w[SK3_USE] ? w[SK3X_PASSES] : 0u;
    if (full_passes) *full_passes = w[SK3_USE] ? w[SK3_PASSES] : 0u;
    return TREXHIP_OK;
}

int trexhip_identify_skip3_ran(trexhip_ctx* ctx, uint32_t* windowed_passes, uint32_t* full_passes) {
    uint32_t w[SK_WORDS];
    if (const int rc = read_skip_words(ctx, "trexhip_identify_skip3_ran", w)) return rc;
    if (windowed_passes) *windowed_passes = w[SK3_USE] ? w[SK3X_RAN] : 0u;
    if (full_passes) *full_passes = w[SK3_USE] ? w[SK3_RAN] : 0u;
    return TREXHIP_OK;
}

int trexhip_identify_skip3_stats(trexhip_ctx* ctx, uint32_t* pairs, uint32_t* listed, uint32_t* passes, uint64_t* bytes_filled) {
    uint32_t w[SK_WORDS];
    if (const int rc = read_skip_words(ctx, "trexhip_identify_skip3_stats", w)) return rc;
    if (pairs) *pairs = w[SK3_PAIRS];
    if (listed) *listed = w[SK3_LISTED];
    // (passes keeps counting by the row rule alone, as skip_stats does: the passes of six pairs the listed pairs make.  Where windowed passes ran
    // the device has not counted those; the host restates them from the bands the call left, with the function the list kernels pack by)
    uint32_t by_rows = w[SK3_PASSES];
    if (passes && w[SK3_USE] && w[SK3X_PASSES]) {
        const Net* net = static_cast<Net*>(ctx->net);
        const int n = (int)(w[SK3_PAIRS] / Skip3Geom::PAIRS);
        std::vector<int2> bands((size_t)n);
        TH_CHECK_HIP(hipMemcpy(bands.data(), net->skip_bands, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost));
        int count = 0;
        for (int c0 = 0; c0 < n; c0 += Skip3Geom::BLOCK) {
            Skip3Pass p{};
            for (int c = c0; c < n && c < c0 + Skip3Geom::BLOCK; ++c) {
                const SkipPairs r = skip3_pairs({bands[(size_t)c].x, bands[(size_t)c].y});      // (windows exist: the empty crop is in range)
                if (r.lo <= r.hi) skip3_add_run(p, count, c * Skip3Geom::PAIRS + r.lo, r.hi - r.lo + 1, [](int, const Skip3Pass&) {});
            }
            skip3_flush(p, count, [](int, const Skip3Pass&) {});
        }
        by_rows = (uint32_t)count;
    }
    if (passes) *passes = w[SK3_USE] ? by_rows : 0u;
    if (bytes_filled) *bytes_filled = (uint64_t)w[SK3_FILLED] * (10 * 128 * 4);
    return TREXHIP_OK;
}

int trexhip_identify_fc1_stats(trexhip_ctx* ctx, uint32_t* rows, uint32_t* listed) {
    uint32_t w[SK_WORDS];
    if (const int rc = read_skip_words(ctx, "trexhip_identify_fc1_stats", w)) return rc;
    const Net* net = static_cast<Net*>(ctx->net);
    uint32_t sum = 0;      // (the lengths are those of the last call that listed: they count only where that was the last call)
    for (int q = 0; q < Skip3Geom::PAIRS && net->last_fc1_n; ++q) sum += w[SK3_FC1_LEN + q];
    if (rows) *rows = (uint32_t)net->last_fc1_n * Skip3Geom::PAIRS;
    if (listed) *listed = sum;
    return TREXHIP_OK;
}

int trexhip_set_identity_precision(trexhip_ctx* ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 3) { set_error("trexhip_set_identity_precision: mode must be one of TREXHIP_CNN_*"); return TREXHIP_E_INVALID; }
    ctx->cnn_mode = mode;
    ctx->prepared.precision_changed();
    return TREXHIP_OK;
}

int trexhip_num_classes(trexhip_ctx* ctx) {
    if (!ctx || !ctx->net) return 0;
    return static_cast<Net*>(ctx->net)->classes;
}

int trexhip_network_version(trexhip_ctx* ctx) {
    if (!ctx || !ctx->net) return 0;
    const Net* net = static_cast<const Net*>(ctx->net);
    return net->arch ? net->arch->plan.spec->id : TREXHIP_NET_V118_3;
}

size_t trexhip_network_blob_bytes(int32_t version, int32_t classes, int32_t channels, int32_t width, int32_t height) {
    return arch_blob_bytes(version, classes, channels, width, height);
}

int trexhip_identify_chunk_crops(trexhip_ctx* ctx, int32_t* crops) {
    if (!ctx || !crops) { set_error("trexhip_identify_chunk_crops: null argument"); return TREXHIP_E_INVALID; }
    const Net* net = static_cast<const Net*>(ctx->net);
    *crops = net && net->arch ? net->arch->plan.chunk : 0;
    return TREXHIP_OK;
}

int trexhip_network_channels(trexhip_ctx* ctx) {
    if (!ctx || !ctx->net) return 0;
    return static_cast<Net*>(ctx->net)->CH;
}

int trexhip_network_image_size(trexhip_ctx* ctx, int32_t* width, int32_t* height) {
    if (!ctx) { set_error("trexhip_network_image_size: null context"); return TREXHIP_E_INVALID; }
    const Net* net = static_cast<const Net*>(ctx->net);
    if (width) *width = net ? net->W : 0;
    if (height) *height = net ? net->H : 0;
    return TREXHIP_OK;
}

}  // extern "C"

namespace trexhip {
void net_free(trexhip_ctx* ctx) {
    ctx->prepared.closed();
    free_net(static_cast<Net*>(ctx->net)); ctx->net = nullptr;
    free_net(static_cast<Net*>(ctx->cat)); ctx->cat = nullptr;
}
}
