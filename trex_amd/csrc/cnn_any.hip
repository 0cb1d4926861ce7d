// cnn_any.hip -- the convolutions of the identity network V118_3 at any individual_image_size but 80x80 (cnn.hip keeps its own
// chain there).  W, H = 8..256 at run time, square or not, CH = 1 or 3, NHWC throughout; every pool floors like nn.MaxPool2d(2).
//
//   k_any_conv1      CH -> 16, exact fp32 on the VALU: one workgroup per (crop, 16 x 16 pooled outputs), u8 patch in LDS
//   k_any_conv<>     conv2 (16 -> 64) / conv3 (64 -> 128) as 25 shifted GEMMs on the matrix cores, the model of k_conv5 (conv_f32.h)
//                    and k_conv5_split (cnn.hip) with a 2-D output tile instead of full-width row bands:
//                      * a tile is 64 pool windows (8 M-tiles of 32 conv pixels, pool-window-major, so the 2x2 max-pool is a max over
//                        four accumulator registers of one lane) shaped 4 x 16, 8 x 8 or 16 x 4 windows -- the host takes the shape
//                        with the fewest tiles for the layer's output; the last row / column of tiles is ragged and masked;
//                      * the input patch of a tile (2 TY + 4) x (2 TX + 4) x 16 channels is at most 432 pixels whatever W is, so the
//                        LDS footprint is fixed per instance (fp16: 57 KB for conv3, bf16: 87 KB, fp32: 90 KB);
//                      * KIND 2 = exact fp32 (v_mfma_f32_32x32x2_f32), 0 = three bf16 pieces (NTERMS 6 or 3), 1 = two fp16 pieces
//                        (3 piece products, scaled weights): the arithmetic of the 80x80 chain's precision modes.
//   The fp16 kernels flag the crop of an activation outside the fp16 range (crop_flags + overflow bit 0); k_guard_plan (cnn.hip)
//   lists those crops and the bf16x6 instances, launched with that plan as their guard, re-run only them.
#include "cnn_net.h"
#include "cnn_split.h"

namespace trexhip {
namespace {

// ------------------------------------------------------------------------------------------------
// conv1: CH -> 16, 5x5 'same' + folded BN + ReLU + floor 2x2 max-pool, exact fp32
// ------------------------------------------------------------------------------------------------
template <int CH>
__global__ __launch_bounds__(256) void k_any_conv1(const uint8_t* __restrict__ crops /*[N][H][W][CH]*/, const float* __restrict__ w /*[CH][25][16]*/,
                                                   const float* __restrict__ bias, float* __restrict__ out /*[N][H/2][W/2][16]*/,
                                                   const int W, const int H, const int tx_n, const int tiles) {
    constexpr int PW = 2 * C1T + 4;
    __shared__ __attribute__((aligned(16))) float wl[CH * 25 * 16];
    __shared__ float img[CH * PW * PW];
    const int crop = blockIdx.x / tiles, t = blockIdx.x - crop * tiles;
    const int ty = t / tx_n, tx = t - ty * tx_n;
    const int y0 = 2 * C1T * ty - 2, x0 = 2 * C1T * tx - 2;
    const uint8_t* src = crops + (size_t)crop * H * W * CH;
    for (int i = threadIdx.x; i < CH * 25 * 16; i += 256) wl[i] = w[i];
    for (int i = threadIdx.x; i < PW * PW * CH; i += 256) {
        const int c = i % CH, p = i / CH, py = p / PW, px = p - py * PW;
        const int iy = y0 + py, ix = x0 + px;
        img[c * PW * PW + p] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? (float)src[((size_t)iy * W + ix) * CH + c] : 0.f;   // predict_numpy: no scaling
    }
    __syncthreads();
    const int Ho = H / 2, Wo = W / 2;
    const int wy = threadIdx.x / C1T, wx = threadIdx.x % C1T;
    const int oy = C1T * ty + wy, ox = C1T * tx + wx;
    if (oy >= Ho || ox >= Wo) return;
    float acc[4][16];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int co = 0; co < 16; ++co) acc[s4][co] = 0.f;
    for (int c = 0; c < CH; ++c) {
        const float* base = img + c * PW * PW + (2 * wy) * PW + 2 * wx;
#pragma unroll 1
        for (int ky = 0; ky < 5; ++ky) {
            float r0[6], r1[6];
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
    float* o = out + (((size_t)crop * Ho + oy) * Wo + ox) * 16;
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

// ------------------------------------------------------------------------------------------------
// conv2 / conv3: 5x5 'same' + folded BN + ReLU + floor 2x2 max-pool on the matrix cores, 2-D output tiles
// ------------------------------------------------------------------------------------------------
constexpr int APMAX = 36 * 12;               // patch pixels of the largest tile shape (4 x 16 or 16 x 4 windows)

template <int KIND> struct AnyK;             // 0 = bf16 (3 pieces), 1 = fp16 (2 pieces), 2 = fp32
template <> struct AnyK<0> { static constexpr int NP = 3; using frag = bf16x8; };
template <> struct AnyK<1> { static constexpr int NP = 2; using frag = f16x8; };
template <> struct AnyK<2> { static constexpr int NP = 1; using frag = float; };

template <int CO, int KIND, int CIC>
struct AnyGeom {
    static constexpr int NP = AnyK<KIND>::NP;
    static constexpr int PSTRIDE = KIND == 2 ? (CIC + 1) * 4 : CIC * 2 + 16;      // bytes per patch pixel (fp32: odd float stride; split: odd multiple of 16)
    static constexpr int PIECE = APMAX * PSTRIDE;                                  // bytes per piece of the patch
    static constexpr int BT = KIND == 2 ? CIC * CO * 4 : NP * (CIC / 8) * CO * 16;   // bytes per weight tile (one tap of one chunk)
    static constexpr int BV = BT / 16;
    static constexpr int BPT = (BV + 511) / 512;
    static constexpr int NT = CO / 32, WM = 8 / NT, TPW = 8 / WM;               // 8 waves: NT along N, WM along M, TPW M-tiles each
    static constexpr int LDS_BYTES = NP * PIECE + 2 * BT;
};

// wp: KIND 2 [CI/CIC][25][CIC][CO] fp32;  KIND 0 / 1 [CI/16][25][NP][2][CO] x 16 B (the pieces of upload_split / upload_split_f16).
// One workgroup per (crop, tile); with a guard (the plan of k_guard_plan) a small grid walks the tiles of the listed crops.
template <int CI, int CO, int KIND, int NTERMS, int CIC>
__global__ __launch_bounds__(512) void k_any_conv(const float* __restrict__ in /*[N][Hi][Wi][CI]*/, const uint4* __restrict__ wp,
                                                  const float* __restrict__ bias, float* __restrict__ out /*[N][Hi/2][Wi/2][CO]*/,
                                                  const int Hi, const int Wi, const int TX, const int tx_n, const int tiles,
                                                  const float out_scale, uint32_t* __restrict__ overflow, uint8_t* __restrict__ crop_flags,
                                                  const uint32_t* __restrict__ guard, const int n_blocks) {
    if (guard && guard[1] == 0u) return;          // re-run pass: only when the fp16 pass flagged something
    using G = AnyGeom<CO, KIND, CIC>;
    using frag = typename AnyK<KIND>::frag;
    static_assert(KIND == 2 || CIC == 16, "the split weights come in 16-channel chunks");
    constexpr int Q4 = CIC / 4, KO = CIC / 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t ldsb[];
    uint8_t* patch = ldsb;
    uint8_t* Bs = ldsb + G::NP * G::PIECE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = wave % G::NT, mg = wave / G::NT;
    const int TY = AW / TX, PW = 2 * TX + 4, PH = 2 * TY + 4;
    const int Ho = Hi / 2, Wo = Wi / 2;
    int aoff[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int p = (mg + G::WM * m) * 32 + j;                        // window-major pixel index of the tile, < 256
        const int wi = p >> 2, sub = p & 3;
        const int wy = wi / TX, wx = wi - wy * TX;
        aoff[m] = ((2 * wy + (sub >> 1)) * PW + (2 * wx + (sub & 1))) * G::PSTRIDE + (KIND == 2 ? h * 4 : h * 16);
    }
    const int n_eff = (guard && guard[1] == 1u) ? (int)guard[0] * tiles : n_blocks;
    for (int blk = blockIdx.x; blk < n_eff; blk += gridDim.x) {
        if (blk != (int)blockIdx.x) __syncthreads();                    // the previous tile's readers are done with the LDS buffers
        const int crop = plan_crop(guard, blk / tiles), t = blk % tiles;
        const int ty = t / tx_n, tx = t - ty * tx_n;
        const int oy0 = ty * TY, ox0 = tx * TX;                         // first pooled output of the tile
        const int iy0 = 2 * oy0 - 2, ix0 = 2 * ox0 - 2;                 // first input pixel of its patch
        f32x16 acc[G::TPW];
#pragma unroll
        for (int m = 0; m < G::TPW; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
        const float* inc = in + (size_t)crop * Hi * Wi * CI;
        bool ovf = false;
        for (int cc = 0; cc < CI / CIC; ++cc) {
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
            const uint4* wsrc = wp + (size_t)cc * 25 * G::BV;
            for (int i = tid; i < G::BV; i += 512) reinterpret_cast<uint4*>(Bs)[i] = wsrc[i];
            __syncthreads();
#pragma unroll 1
            for (int tap = 0; tap < 25; ++tap) {                        // (unrolled, the fp16 conv3 instance spills: 104 VGPRs)
                const int buf = tap & 1;
                uint4 nb[G::BPT];
                if (tap < 24) {
#pragma unroll
                    for (int u = 0; u < G::BPT; ++u) { const int i = tid + u * 512; if (i < G::BV) nb[u] = wsrc[(size_t)(tap + 1) * G::BV + i]; }
                }
                const uint8_t* asrc = patch + ((tap / 5) * PW + (tap % 5)) * G::PSTRIDE;
                if constexpr (KIND == 2) {
                    const float* bsrc = reinterpret_cast<const float*>(Bs + buf * G::BT) + h * CO + n * 32 + j;
#pragma unroll
                    for (int t2 = 0; t2 < CIC / 2; ++t2) {                // input channel 2 t2 + h of the chunk
                        const float b = bsrc[2 * t2 * CO];
#pragma unroll
                        for (int m = 0; m < G::TPW; ++m) {
                            const float a = *reinterpret_cast<const float*>(asrc + aoff[m] + 8 * t2);
                            acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[m], 0, 0, 0);
                        }
                    }
                } else {
                    const uint8_t* bsrc = Bs + buf * G::BT + (h * CO + n * 32 + j) * 16;
                    const frag b1 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc));
                    const frag b2 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc + KO * CO * 16));
                    frag b3 = b1;
                    if constexpr (G::NP == 3) b3 = __builtin_bit_cast(frag, *reinterpret_cast<const uint4*>(bsrc + 2 * KO * CO * 16));
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
                if (tap < 24) {
#pragma unroll
                    for (int u = 0; u < G::BPT; ++u) { const int i = tid + u * 512; if (i < G::BV) reinterpret_cast<uint4*>(Bs + (buf ^ 1) * G::BT)[i] = nb[u]; }
                }
                __syncthreads();
            }
        }
        if (KIND == 1 && __any(ovf) && lane == 0) { crop_flags[crop] = 1; atomicOr(overflow, 1u); }     // the crop is known: k_guard_plan lists it
        // epilogue: lane (j, h) holds for g = 0..3 the four pixels of window mt * 8 + 2 g + h, channel n * 32 + j
        const int co = n * 32 + j;
        const float bz = bias[co];
        float* oc = out + (size_t)crop * Ho * Wo * CO;
#pragma unroll
        for (int m = 0; m < G::TPW; ++m) {
            const int mt = mg + G::WM * m;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int wi = mt * 8 + 2 * g + h;
                const int wy = wi / TX, wx = wi - wy * TX;
                const int oy = oy0 + wy, ox = ox0 + wx;
                if (oy >= Ho || ox >= Wo) continue;                     // ragged edge of the layer
                const float v = fmaxf(fmaxf(acc[m][4 * g], acc[m][4 * g + 1]), fmaxf(acc[m][4 * g + 2], acc[m][4 * g + 3]));
                oc[((size_t)oy * Wo + ox) * CO + co] = fmaxf(v * out_scale + bz, 0.f);      // out_scale undoes the weight scaling (fp16 pieces)
            }
        }
    }
}

// the four precision instances of a layer, each stated once; the bf16x6 one also runs the guarded re-run
using AnyKern = decltype(Kern(k_any_conv<16, 64, 2, 1, 16>, 512));
template <int CI, int CO, int KIND, int NTERMS, int CIC>
AnyKern any_kern() { return Kern(k_any_conv<CI, CO, KIND, NTERMS, CIC>, 512, AnyGeom<CO, KIND, CIC>::LDS_BYTES); }
struct AnyLayer { AnyKern by_mode[4]; };     // indexed by TREXHIP_CNN_*: FP32, BF16X6, BF16X3, FP16X3
const AnyLayer ANY_CONV[2] = {{{any_kern<16, 64, 2, 1, 16>(), any_kern<16, 64, 0, 6, 16>(), any_kern<16, 64, 0, 3, 16>(), any_kern<16, 64, 1, 3, 16>()}},
                              {{any_kern<64, 128, 2, 1, 32>(), any_kern<64, 128, 0, 6, 16>(), any_kern<64, 128, 0, 3, 16>(), any_kern<64, 128, 1, 3, 16>()}}};
const ByChannels ANY_CONV1{Kern(k_any_conv1<1>, 256), Kern(k_any_conv1<3>, 256)};

}  // namespace

void any_conv1(hipStream_t s, const Net& net, const CnnPlan& p, const uint8_t* d_crops) {
    ANY_CONV1[net.CH](s, p.conv1_grid, d_crops, net.w1, net.b1, net.act1, net.W, net.H, p.tx1, p.t1);
}

void any_conv(hipStream_t s, const Net& net, const CnnPlan& p, const int layer, const int mode, const uint32_t* guard) {
    const bool c2 = layer == 2, h16 = mode == TREXHIP_CNN_FP16X3;
    const AnyTiles& tl = c2 ? p.t2 : p.t3;
    const Launch& l = guard ? (c2 ? p.r_conv2 : p.r_conv3) : (c2 ? p.conv2 : p.conv3);
    const void* w = mode == TREXHIP_CNN_FP32 ? (c2 ? (const void*)net.w2 : net.w3) : h16 ? (c2 ? net.w2h : net.w3h) : (c2 ? net.w2s : net.w3s);
    ANY_CONV[layer - 2].by_mode[mode](s, l.grid, c2 ? net.act1 : net.act2, w, c2 ? net.b2 : net.b3, c2 ? net.act2 : net.act3, net.H / (c2 ? 2 : 4),
                                      net.W / (c2 ? 2 : 4), tl.TX, tl.tx_n, tl.tiles, h16 ? (c2 ? net.inv2h : net.inv3h) : 1.f, net.ovf(OVF_RANGE), net.d_ovfc,
                                      guard, l.items);
}

}  // namespace trexhip
