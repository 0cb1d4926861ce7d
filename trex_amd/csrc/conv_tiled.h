// conv_tiled.h -- the tiled convolutions of the identity networks away from the tuned 80x80 chain, each stated once: the any-size V118_3 chain
// (cnn_any.hip) and the v100 / v110 / v119 / v200 / category chains (cnn_arch.hip) are instances of the two bodies below, and the three
// plan kernels (k_guard_plan, k_head_small: cnn.hip; k_arch_guard_plan: cnn_arch.hip) of guard_plan.  NHWC fp32 activations, every pool floors
// like nn.MaxPool2d(2).
//
//   conv1_tiled    first layer, u8 crops -> fp32, T x T taps, exact fp32 on the VALU: one workgroup per (crop, 16 x 16 windows of 2 x 2 conv
//                  pixels) and block of 16 output channels, the u8 patch in LDS, one window per thread
//   conv_tiled     every further convolution as T * T shifted GEMMs on the matrix cores, after k_conv5 (conv_f32.h) and k_conv5_split
//                  (cnn.hip), with a 2-D output tile instead of full-width row bands:
//                    * a tile is 64 windows of 2 x 2 conv pixels (8 M-tiles of 32 conv pixels, window-major, so the 2x2 max-pool is a max
//                      over four accumulator registers of one lane) shaped 4 x 16, 8 x 8 or 16 x 4 windows -- the host takes the shape with
//                      the fewest tiles for the layer's output (any_tiles, cnn_geom.h); the last row / column of tiles is ragged and masked;
//                    * the input patch of a tile (2 TY + T - 1) x (2 TX + T - 1) pixels x CIC channels is at most 432 pixels whatever W is,
//                      so the LDS footprint is fixed per instance (TileGeom);
//                    * KIND 2 = exact fp32 (v_mfma_f32_32x32x2_f32), 0 = three bf16 pieces (NTERMS 6 or 3), 1 = two fp16 pieces (3 piece
//                      products, scaled weights): the arithmetic of the 80x80 chain's precision modes (cnn_split.h).
//                  The fp16 instances flag the crop of an activation outside the fp16 range (crop_flags + overflow bit 0); guard_plan lists
//                  those crops and the bf16x6 instances, launched with that plan as their guard, re-run only them.
//
// What an instance fixes at compile time and what it takes as a kernel argument is stated by its policy (TiledFixed / TiledArgs): the parts
// only one side has -- channel block on the grid's y, affine behind the pool, unpooled store -- sit under `if constexpr (P::ARGS)`.
// The bodies are inlined into `__global__` wrappers whose pointer parameters are `__restrict__`; the two convolution bodies do not repeat the
// qualifier (with it the any-size conv2 instances come out a few instructions longer than the stand-alone kernels they replace).
#pragma once
#include "cnn_split.h"

namespace trexhip {

// ------------------------------------------------------------------------------------------------
// policies
// ------------------------------------------------------------------------------------------------
// V118_3 at any size: channels are the instance's, 5 x 5 taps, pool always on, one channel block, no affine behind the pool
template <int CI_, int CO_>
struct TiledFixed {
    static constexpr bool ARGS = false;
    static constexpr int CI = CI_, CO = CO_, taps = 5, pool = 1;
};
// the layer tables of cnn_arch_plan.h: channels, taps (3 or 5) and pool (0 / 1) are kernel arguments, the block of output channels is the
// grid's y, and relu((x + bias) * s + t) puts an affine BEHIND the pool
struct TiledArgs {
    static constexpr bool ARGS = true;
    int CI, CO, taps, pool;
    const float *sv, *tv;
};

// ------------------------------------------------------------------------------------------------
// first layer: CH -> 16 channels of one block, T x T 'same', optional floor 2x2 max-pool, exact fp32
// ------------------------------------------------------------------------------------------------
// One thread per 2 x 2 window of conv pixels, 16 x 16 windows per workgroup.  LDS: (CH * T * T * 16 + CH * PW * PW) * 4 bytes, PW = 32 + T - 1
// (3 channels, 5 taps: 4800 + 15552 = 20352 B); 64 accumulators per thread
// NORM (the category network, trex_learn_category.py:289, :435 "torch.tensor(images, float32) / 127.5 - 1"): a pixel inside the crop is staged as
//     __fsub_rn(__fdiv_rn((float)byte, 127.5f), 1.0f)      -- a true fp32 division, then an fp32 subtraction, each rounded on its own --
// which is what torch's CPU and what numpy give for all 256 bytes (a multiply by the rounded reciprocal differs at 111 of them, a fused multiply-
// subtract at 205: tests/test_category_ref.py); a pixel outside it as 0, because the reference pads the NORMALISED image with zeros.  The offset
// can therefore not live in the bias.
// w: [CO/16][CH][T*T][16]; out: [N][Ho][Wo][CO].  The policy's CI is not read: the layer's input channels are CH.
template <int CH, int T, bool NORM, class P>
__device__ __forceinline__ void conv1_tiled(const P p, const uint8_t* crops /*[N][H][W][CH]*/, const float* w, const float* bias,
                                            float* out, const int W, const int H, const int tx_n, const int tiles) {
    constexpr int PW = 2 * C1T + T - 1, PAD = T / 2, T2 = T * T;
    __shared__ __attribute__((aligned(16))) float wl[CH * T2 * 16];
    __shared__ float img[CH * PW * PW];
    const int crop = blockIdx.x / tiles, t = blockIdx.x - crop * tiles;
    const int ty = t / tx_n, tx = t - ty * tx_n;
    const int y0 = 2 * C1T * ty - PAD, x0 = 2 * C1T * tx - PAD;
    const uint8_t* src = crops + (size_t)crop * H * W * CH;
    const float* wg = w;
    int cb = 0;                                                          // first output channel of this workgroup
    if constexpr (P::ARGS) { wg += (size_t)blockIdx.y * CH * T2 * 16; cb = blockIdx.y * 16; }
    for (int i = threadIdx.x; i < CH * T2 * 16; i += 256) wl[i] = wg[i];
    for (int i = threadIdx.x; i < PW * PW * CH; i += 256) {
        const int c = i % CH, px = i / CH, py = px / PW, pxx = px - py * PW;
        const int iy = y0 + py, ix = x0 + pxx;
        const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const size_t at = ((size_t)iy * W + ix) * CH + c;
        if constexpr (NORM) img[c * PW * PW + px] = inside ? __fsub_rn(__fdiv_rn((float)src[at], 127.5f), 1.0f) : 0.f;     // zero padding of the normalised image
        else img[c * PW * PW + px] = inside ? (float)src[at] : 0.f;                                                         // predict_numpy: no scaling
    }
    __syncthreads();
    const int wy = threadIdx.x / C1T, wx = threadIdx.x % C1T;
    const int oy = C1T * ty + wy, ox = C1T * tx + wx;                   // the thread's window: pooled, its output
    const int py0 = 2 * oy, px0 = 2 * ox;                               // its first conv pixel
    const int Ho = H / 2, Wo = W / 2;
    if constexpr (P::ARGS) { if (py0 >= H || px0 >= W) return; }        // ragged edge
    else if (oy >= Ho || ox >= Wo) return;                              // ... always pooled: the odd last row / column too, which the floor drops
    float acc[4][16];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int co = 0; co < 16; ++co) acc[s4][co] = 0.f;
    for (int c = 0; c < CH; ++c) {
        const float* base = img + c * PW * PW + (2 * wy) * PW + 2 * wx;
#pragma unroll 1
        for (int ky = 0; ky < T; ++ky) {
            float r0[T + 1], r1[T + 1];                                 // two input rows feed output rows 0 and 1 of the window
#pragma unroll
            for (int b6 = 0; b6 < T + 1; ++b6) { r0[b6] = base[ky * PW + b6]; r1[b6] = base[(ky + 1) * PW + b6]; }
#pragma unroll
            for (int kx = 0; kx < T; ++kx) {
                const float4* wt = reinterpret_cast<const float4*>(wl + (c * T2 + ky * T + kx) * 16);
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
    // relu(x + bias), with the affine of the policy behind the bias
    auto act = [&](const float x, const int co) {
        if constexpr (P::ARGS) return fmaxf((x + bias[co]) * p.sv[co] + p.tv[co], 0.f);
        else return fmaxf(x + bias[co], 0.f);
    };
    if (p.pool) {
        if (oy >= Ho || ox >= Wo) return;                                // the odd last row / column is dropped by the floor
        float* o = out + (((size_t)crop * Ho + oy) * Wo + ox) * p.CO + cb;
#pragma unroll
        for (int co = 0; co < 16; co += 4) {
            float4 v;
            float* vv = &v.x;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float m = fmaxf(fmaxf(acc[0][co + q], acc[1][co + q]), fmaxf(acc[2][co + q], acc[3][co + q]));
                vv[q] = act(m, cb + co + q);
            }
            *reinterpret_cast<float4*>(o + co) = v;
        }
    } else {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int py = py0 + (s4 >> 1), px = px0 + (s4 & 1);
            if (py >= H || px >= W) continue;
            float* o = out + (((size_t)crop * H + py) * W + px) * p.CO + cb;
#pragma unroll
            for (int co = 0; co < 16; co += 4) {
                float4 v;
                float* vv = &v.x;
#pragma unroll
                for (int q = 0; q < 4; ++q) vv[q] = act(acc[s4][co + q], cb + co + q);
                *reinterpret_cast<float4*>(o + co) = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// every further convolution: T x T 'same' on the matrix cores, 2-D tiles of 64 windows of 2 x 2 conv pixels
// ------------------------------------------------------------------------------------------------
constexpr int APMAX = 36 * 12;               // patch pixels of the largest tile shape at 5 taps (4 x 16 or 16 x 4 windows); 3 taps: 34 * 10

template <int KIND> struct TileK;            // 0 = bf16 (3 pieces), 1 = fp16 (2 pieces), 2 = fp32
template <> struct TileK<0> { static constexpr int NP = 3; using frag = bf16x8; };
template <> struct TileK<1> { static constexpr int NP = 2; using frag = f16x8; };
template <> struct TileK<2> { static constexpr int NP = 1; using frag = float; };

// per instance: LDS bytes and accumulator registers.  COB output channels per workgroup; input channels are staged CIC at a time: 16, but 32
// in the any-size fp32 conv3 -- the chunk is part of the order of the fp32 sums, so it is the instance's and not derived here.  At CIC 16:
//   COB 128: fp32 29376 + 16384 = 45760 B, bf16 62208 + 24576 = 86784 B, fp16 41472 + 16384 = 57856 B; 4 M-tiles per wave = 64 accumulators
//   COB  64: fp32 37568, bf16 74496, fp16 49664 B; 32 accumulators          COB 32: fp32 33472, bf16 68352, fp16 45568 B; 16 accumulators
template <int COB, int KIND, int CIC>
struct TileGeom {
    static constexpr int NP = TileK<KIND>::NP;
    static constexpr int PSTRIDE = KIND == 2 ? (CIC + 1) * 4 : CIC * 2 + 16;      // bytes per patch pixel (fp32: odd float stride; split: odd multiple of 16)
    static constexpr int PIECE = APMAX * PSTRIDE;                                  // bytes per piece of the patch
    static constexpr int BT = KIND == 2 ? CIC * COB * 4 : NP * (CIC / 8) * COB * 16;   // bytes per weight tile (one tap of one chunk of one block)
    static constexpr int BV = BT / 16;
    static constexpr int BPT = (BV + 511) / 512;
    static constexpr int NT = COB / 32, WM = 8 / NT, TPW = 8 / WM;                // 8 waves: NT along N, WM along M, TPW M-tiles each
    static constexpr int ACC = TPW * 16;
    static constexpr int LDS_BYTES = NP * PIECE + 2 * BT;
    static_assert(COB == 32 || COB == 64 || COB == 128, "channel block");
    static_assert(KIND == 2 || CIC == 16, "the split weights come in 16-channel chunks");
    static_assert(LDS_BYTES <= 160 * 1024 && ACC <= 128, "LDS / accumulators");
};

// wp: [CO/COB][CI/CIC][T*T] weight tiles: KIND 2 [CIC][COB] fp32; KIND 0 / 1 [NP][2][COB] x 16 B (the pieces of upload_split / upload_split_f16,
// pack_arch_bf16x3 / pack_arch_f16x2).  in: [N][Hi][Wi][CI]; out: [N][Ho][Wo][CO].
// Grid (items, CO / COB): one workgroup per (crop, tile) and channel block; with a guard (the plan of guard_plan) the x grid strides over the
// tiles of the listed crops.
// The epilogue: relu(max_window(conv) * out_scale + bias[co]), out_scale undoing the weight scaling of the fp16 pieces; with TiledArgs
// relu((.. + bias[co]) * s[co] + t[co]) -- the affine BEHIND the pool, which v110 needs (its BatchNorm follows the max-pool and its scale may
// be negative); v119 / v200 fold their BatchNorm into weights and bias (s = 1, t = 0), v100 has none -- and without a pool every conv pixel.
template <int COB, int KIND, int NTERMS, int CIC, class P>
__device__ __forceinline__ void conv_tiled(const P p, const float* in, const uint4* wp, const float* bias, float* out,
                                           const int Hi, const int Wi, const int TX, const int tx_n, const int tiles, const float out_scale,
                                           uint32_t* overflow, uint8_t* crop_flags, const uint32_t* guard, const int n_blocks) {
    if (guard && guard[1] == 0u) return;          // re-run pass: only when the fp16 pass flagged something
    using G = TileGeom<COB, KIND, CIC>;
    using frag = typename TileK<KIND>::frag;
    constexpr int Q4 = CIC / 4, KO = CIC / 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t ldsb[];
    uint8_t* patch = ldsb;
    uint8_t* Bs = ldsb + G::NP * G::PIECE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = wave % G::NT, mg = wave / G::NT;
    const int CI = p.CI, CO = p.CO, taps = p.taps;
    const int T2 = taps * taps, pad = taps >> 1;
    const int TY = AW / TX, PW = 2 * TX + taps - 1, PH = 2 * TY + taps - 1;
    const int Ho = p.pool ? Hi / 2 : Hi, Wo = p.pool ? Wi / 2 : Wi;
    const int ncc = CI / CIC;
    int cb = 0;                                                         // first output channel of this workgroup
    if constexpr (P::ARGS) { wp += (size_t)blockIdx.y * ncc * T2 * G::BV; cb = blockIdx.y * COB; }
    int aoff[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int px = (mg + G::WM * m) * 32 + j;                       // window-major pixel index of the tile, < 256
        const int wi = px >> 2, sub = px & 3;
        const int wy = wi / TX, wx = wi - wy * TX;
        aoff[m] = ((2 * wy + (sub >> 1)) * PW + (2 * wx + (sub & 1))) * G::PSTRIDE + (KIND == 2 ? h * 4 : h * 16);
        // TiledFixed: the offset stays one value.  Left to itself the compiler splits it there into a per-tile and a per-lane term and adds the
        // three of them in every tap (conv3: one VALU add more per tile and tap and 2 more VGPRs than the sum formed here)
        if constexpr (!P::ARGS) asm volatile("" : "+v"(aoff[m]));
    }
    const int n_eff = (guard && guard[1] == 1u) ? (int)guard[0] * tiles : n_blocks;
    for (int blk = blockIdx.x; blk < n_eff; blk += gridDim.x) {
        if (blk != (int)blockIdx.x) __syncthreads();                    // the previous tile's readers are done with the LDS buffers
        const int crop = plan_crop(guard, blk / tiles), t = blk % tiles;
        const int ty = t / tx_n, tx = t - ty * tx_n;
        const int oy0 = ty * TY, ox0 = tx * TX;                         // first window of the tile
        const int iy0 = 2 * oy0 - pad, ix0 = 2 * ox0 - pad;             // first input pixel of its patch
        f32x16 acc[G::TPW];
#pragma unroll
        for (int m = 0; m < G::TPW; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
        const float* inc = in + (size_t)crop * Hi * Wi * CI;
        bool ovf = false;
        for (int cc = 0; cc < ncc; ++cc) {
            __syncthreads();
            for (int idx = tid; idx < PH * PW * Q4; idx += 512) {
                const int q = idx % Q4, px = idx / Q4;
                const int py = px / PW, pxx = px - py * PW;
                const int iy = iy0 + py, ix = ix0 + pxx;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);             // zero padding ('same'), and the rows / columns past a ragged edge
                if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi)
                    v = *reinterpret_cast<const float4*>(inc + ((size_t)iy * Wi + ix) * CI + cc * CIC + q * 4);
                if constexpr (KIND == 2) {
                    float* d = reinterpret_cast<float*>(patch + px * G::PSTRIDE) + q * 4;
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                } else {
                    uint32_t a1[4], a2[4], a3[4];
                    if constexpr (KIND == 0) {
                        split3(v.x, a1[0], a2[0], a3[0]); split3(v.y, a1[1], a2[1], a3[1]);
                        split3(v.z, a1[2], a2[2], a3[2]); split3(v.w, a1[3], a2[3], a3[3]);
                    } else {
                        split2h(v.x, a1[0], a2[0], ovf); split2h(v.y, a1[1], a2[1], ovf);
                        split2h(v.z, a1[2], a2[2], ovf); split2h(v.w, a1[3], a2[3], ovf);
                    }
                    uint8_t* d = patch + px * G::PSTRIDE + q * 8;
                    *reinterpret_cast<uint2*>(d) = make_uint2(a1[0] | (a1[1] << 16), a1[2] | (a1[3] << 16));
                    *reinterpret_cast<uint2*>(d + G::PIECE) = make_uint2(a2[0] | (a2[1] << 16), a2[2] | (a2[3] << 16));
                    if constexpr (KIND == 0) *reinterpret_cast<uint2*>(d + 2 * G::PIECE) = make_uint2(a3[0] | (a3[1] << 16), a3[2] | (a3[3] << 16));
                }
            }
            const uint4* wsrc = wp + (size_t)cc * T2 * G::BV;
            for (int i = tid; i < G::BV; i += 512) reinterpret_cast<uint4*>(Bs)[i] = wsrc[i];
            __syncthreads();
            int ky = 0, kx = 0;                                         // TiledArgs: the tap's row and column, counted
#pragma unroll 1
            for (int tap = 0; tap < T2; ++tap) {                        // (unrolled, the fp16 conv3 instance of V118_3 spills: 104 VGPRs)
                const int buf = tap & 1;
                uint4 nb[G::BPT];
                if (tap < T2 - 1) {
#pragma unroll
                    for (int u = 0; u < G::BPT; ++u) { const int i = tid + u * 512; if (i < G::BV) nb[u] = wsrc[(size_t)(tap + 1) * G::BV + i]; }
                }
                const uint8_t* asrc = patch + (P::ARGS ? ky * PW + kx : (tap / taps) * PW + tap % taps) * G::PSTRIDE;     // TiledFixed: divided by the constant
                if constexpr (KIND == 2) {
                    const float* bsrc = reinterpret_cast<const float*>(Bs + buf * G::BT) + h * COB + n * 32 + j;
#pragma unroll
                    for (int t2 = 0; t2 < CIC / 2; ++t2) {                // input channel 2 t2 + h of the chunk
                        const float b = bsrc[2 * t2 * COB];
#pragma unroll
                        for (int m = 0; m < G::TPW; ++m) {
                            const float a = *reinterpret_cast<const float*>(asrc + aoff[m] + 8 * t2);
                            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[m], 0, 0, 0);
                        }
                    }
                } else {
                    const uint8_t* bsrc = Bs + buf * G::BT + (h * COB + n * 32 + j) * 16;
                    const frag b1 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc));
                    const frag b2 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc + KO * COB * 16));
                    frag b3 = b1;
                    if constexpr (G::NP == 3) b3 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc + 2 * KO * COB * 16));
#pragma unroll
                    for (int m = 0; m < G::TPW; ++m) {
                        const frag p1 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(asrc + aoff[m]));
                        const frag p2 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(asrc + aoff[m] + G::PIECE));
                        if constexpr (KIND == 0 && NTERMS == 6) {        // smallest products first: a3b1 a2b2 a1b3 a2b1 a1b2 a1b1
                            const frag p3 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(asrc + aoff[m] + 2 * G::PIECE));
                            acc[m] = mfma16(p3, b1, acc[m]); acc[m] = mfma16(p2, b2, acc[m]); acc[m] = mfma16(p1, b3, acc[m]);
                        }
                        acc[m] = mfma16(p2, b1, acc[m]); acc[m] = mfma16(p1, b2, acc[m]); acc[m] = mfma16(p1, b1, acc[m]);
                    }
                }
                if (tap < T2 - 1) {
#pragma unroll
                    for (int u = 0; u < G::BPT; ++u) { const int i = tid + u * 512; if (i < G::BV) reinterpret_cast<uint4*>(Bs + (buf ^ 1) * G::BT)[i] = nb[u]; }
                }
                if constexpr (P::ARGS) { if (++kx == taps) { kx = 0; ++ky; } }
                __syncthreads();
            }
        }
        if (KIND == 1 && __any(ovf) && lane == 0) { crop_flags[crop] = 1; atomicOr(overflow, 1u); }     // the crop is known: the plan lists it
        // epilogue: lane (j, h) holds for g = 0..3 the four pixels of window mt * 8 + 2 g + h, channel cb + n * 32 + j
        const int co = cb + n * 32 + j;
        const float bz = bias[co];
        float sc, sh;
        if constexpr (P::ARGS) { sc = p.sv[co]; sh = p.tv[co]; }
        auto act = [&](const float x) {
            if constexpr (P::ARGS) return fmaxf((x * out_scale + bz) * sc + sh, 0.f);
            else return fmaxf(x * out_scale + bz, 0.f);
        };
        float* oc = out + (size_t)crop * Ho * Wo * CO;
#pragma unroll
        for (int m = 0; m < G::TPW; ++m) {
            const int mt = mg + G::WM * m;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int wi = mt * 8 + 2 * g + h;
                const int wy = wi / TX, wx = wi - wy * TX;
                if (p.pool) {
                    const int oy = oy0 + wy, ox = ox0 + wx;
                    if (oy >= Ho || ox >= Wo) continue;                 // ragged edge of the layer
                    oc[((size_t)oy * Wo + ox) * CO + co] = act(fmaxf(fmaxf(acc[m][4 * g], acc[m][4 * g + 1]), fmaxf(acc[m][4 * g + 2], acc[m][4 * g + 3])));
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int py = 2 * (oy0 + wy) + (q >> 1), px = 2 * (ox0 + wx) + (q & 1);
                        if (py >= Hi || px >= Wi) continue;
                        oc[((size_t)py * Wi + px) * CO + co] = act(acc[m][4 * g + q]);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// fp16 range guard, per crop.  The fp16 chains raise overflow[0] when an activation leaves the range its fp16 pieces can hold and, where they
// know the crop, flags[crop].  guard_plan turns the flags into a plan for the bf16 re-run:
//   plan[0] = number of listed crops, plan[1] = mode (0 nothing to do, 1 the listed crops only, 2 every crop), plan[2 ..] = the list.
// The re-run kernels take the plan as their guard: item i of a launch is crop plan[2 + i] in list mode (plan_crop, cnn_split.h).  One
// out-of-range crop in 25600 costs the launches of the re-run chain and its own crop, not a second pass over the whole batch.
// ------------------------------------------------------------------------------------------------
// (called by every thread of ONE workgroup of NT threads; `cnt` is that workgroup's shared counter.)  The last reader of the range flag and of the
// persistent convolutions' pass counters (overflow[1], overflow[2]) hands all three back zeroed for the next forward pass: no memset in front of
// a pass.  The networks of cnn_arch.hip have those two words in their d_ovf as well, never count passes in them and never raise bit 1, so the
// zeroing and the bit's test change nothing there.  stats (those networks): two words of the call that what was planned is added to --
// [0] += crops listed, [1] = 1 when every crop of a chunk is re-run.
template <int NT>
__device__ __forceinline__ void guard_plan(uint32_t* __restrict__ overflow, uint8_t* __restrict__ flags, const int n, uint32_t* __restrict__ plan, uint32_t& cnt,
                                           uint32_t* __restrict__ stats = nullptr) {
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const uint32_t raised = overflow[0];      // bit 0: something left the fp16 range; bit 1: a kernel that cannot name the crop saw it
    if (raised == 0u) {
        // (flags of an aborted earlier pass would enlarge a later plan: what is there is cleared even when nothing was raised)
        for (int i = threadIdx.x; i < n; i += NT) if (flags[i]) flags[i] = 0;
        if (threadIdx.x == 0) { plan[0] = 0; plan[1] = 0; overflow[1] = 0u; overflow[2] = 0u; }
        return;
    }
    for (int i = threadIdx.x; i < n; i += NT)
        if (flags[i]) {
            flags[i] = 0;
            const uint32_t k = atomicAdd(&cnt, 1u);
            if (k < (uint32_t)FB_MAX) plan[2 + k] = (uint32_t)i;
        }
    __syncthreads();
    // an unattributed flag re-runs every crop even when other crops ARE listed: a crop that left the range in k_conv1_wpre / k_conv2_wpre2 (the
    // 3-channel chain) must not keep its fp16 result because fc1 happened to flag another crop of the batch
    if (threadIdx.x == 0) {
        const bool whole = (raised & 2u) || cnt == 0u || cnt > (uint32_t)FB_MAX;
        plan[0] = whole ? 0u : cnt; plan[1] = whole ? 2u : 1u;
        if (stats) { if (whole) stats[1] = 1u; else stats[0] += cnt; }
        overflow[0] = 0u; overflow[1] = 0u; overflow[2] = 0u;
    }
}

}  // namespace trexhip
