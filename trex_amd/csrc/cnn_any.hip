// cnn_any.hip -- the convolutions of the identity network V118_3 at any individual_image_size but 80x80 (cnn.hip keeps its own
// chain there).  W, H = 8..256 at run time, square or not, CH = 1 or 3, NHWC throughout; every pool floors like nn.MaxPool2d(2).
//
//   k_any_conv1      CH -> 16, exact fp32 on the VALU: conv1_tiled (conv_tiled.h) at 5 taps, pooled, one block of 16 channels
//   k_any_conv<>     conv2 (16 -> 64) / conv3 (64 -> 128) on the matrix cores: conv_tiled (conv_tiled.h) with CI, CO, the 25 taps and the
//                    pool as constants, one channel block (COB = CO) and no affine behind the pool.  Input channels are staged 16 at a time,
//                    32 in the fp32 conv3; LDS per instance: fp16 57 KB for conv3, bf16 87 KB, fp32 90 KB.
//   The fp16 kernels flag the crop of an activation outside the fp16 range (crop_flags + overflow bit 0); k_guard_plan (cnn.hip)
//   lists those crops and the bf16x6 instances, launched with that plan as their guard, re-run only them.
#include "cnn_net.h"
#include "conv_tiled.h"

namespace trexhip {
namespace {

template <int CH>
__global__ __launch_bounds__(256) void k_any_conv1(const uint8_t* __restrict__ crops /*[N][H][W][CH]*/, const float* __restrict__ w /*[CH][25][16]*/,
                                                   const float* __restrict__ bias, float* __restrict__ out /*[N][H/2][W/2][16]*/,
                                                   const int W, const int H, const int tx_n, const int tiles) {
    conv1_tiled<CH, 5, false>(TiledFixed<CH, 16>{}, crops, w, bias, out, W, H, tx_n, tiles);
}

// wp: KIND 2 [CI/CIC][25][CIC][CO] fp32;  KIND 0 / 1 [CI/16][25][NP][2][CO] x 16 B (the pieces of upload_split / upload_split_f16).
// One workgroup per (crop, tile); with a guard (the plan of k_guard_plan) a small grid walks the tiles of the listed crops.
template <int CI, int CO, int KIND, int NTERMS, int CIC>
__global__ __launch_bounds__(512) void k_any_conv(const float* __restrict__ in /*[N][Hi][Wi][CI]*/, const uint4* __restrict__ wp,
                                                  const float* __restrict__ bias, float* __restrict__ out /*[N][Hi/2][Wi/2][CO]*/,
                                                  const int Hi, const int Wi, const int TX, const int tx_n, const int tiles,
                                                  const float out_scale, uint32_t* __restrict__ overflow, uint8_t* __restrict__ crop_flags,
                                                  const uint32_t* __restrict__ guard, const int n_blocks) {
    conv_tiled<CO, KIND, NTERMS, CIC>(TiledFixed<CI, CO>{}, in, wp, bias, out, Hi, Wi, TX, tx_n, tiles, out_scale, overflow, crop_flags, guard, n_blocks);
}

// the four precision instances of a layer, each stated once; the bf16x6 one also runs the guarded re-run
using AnyKern = decltype(Kern(k_any_conv<16, 64, 2, 1, 16>, 512));
template <int CI, int CO, int KIND, int NTERMS, int CIC>
AnyKern any_kern() { return Kern(k_any_conv<CI, CO, KIND, NTERMS, CIC>, 512, TileGeom<CO, KIND, CIC>::LDS_BYTES); }
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
