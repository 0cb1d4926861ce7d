// train_any.h -- the launches of the size-following training kernels (train_any.hip), as train.hip's walk calls them: the convolutions at any
// individual_image_size but 80x80, the BN / pool and fc1 kernels at every size.  Every grid comes from the TrainAnyGeom of the trainer (train_geom.h); everything is queued on the given stream, nothing synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "train_geom.h"

namespace trexhip {

int tany_attrs();      // the dynamic-LDS limits of the convolution instances (per device, like trainer_attrs)

// Every convolution below has g.taps x g.taps taps (5, or the category network's 3: its conv1 pair then normalises x as x / 127.5 - 1 and pads with 0).
// conv1 forward: x [n][H][W][CH] -> z1 [n][H][W][16] = convolution + bias
void tany_conv1(hipStream_t s, const TrainAnyGeom& g, int n, const float* x, const float* w, const float* b, float* z);
// conv2 / conv3 (layer 1 / 2) forward: in [n][h][w][CI] -> z [n][h][w][C] = convolution + bias; w in the parameter layout [CI / CIC][taps^2][CIC][C]
void tany_conv_fwd(hipStream_t s, const TrainAnyGeom& g, int layer, int n, const float* in, const float* w, const float* bias, float* z);
// ... data gradient: dz [n][h][w][C] -> da of the block below [n][h][w][CI], on k_t_repack_bwd's flipped + transposed weights
void tany_conv_dgrad(hipStream_t s, const TrainAnyGeom& g, int layer, int n, const float* dz, const float* wb, float* da);
// ... weight gradient: part[g.wg_shares(layer, n)][taps^2][CI][C], summed by k_t_wgrad_reduce
void tany_wgrad(hipStream_t s, const TrainAnyGeom& g, int layer, int n, const float* a, const float* dz, float* part);
// conv1 weight gradient: part[n * g.wg1_tiles][CH][taps^2][16], summed by k_t_reduce
void tany_wgrad1(hipStream_t s, const TrainAnyGeom& g, int n, const float* x, const float* dz, float* part);

// BN + ReLU + floor 2x2 max-pool + channel dropout of a plane of h x w pixels with C = 16, 64 or 128 channels, and the way back
// creal = 0: Dropout2d, keep [n][C].  creal > 0: element-wise dropout (nn.Dropout on the pooled plane), keep [n][h / 2][w / 2][creal], one byte per
// pooled element, and a channel >= creal gives activation 0 and gradient 0 whatever its slots hold
void tany_bn_pool(hipStream_t s, int C, const float* z, const float* mean, const float* invstd, const float* g, const float* be, const uint8_t* keep, float scale,
                  float* a, int n, int h, int w, int creal = 0);
void tany_pool_bwd_stats(hipStream_t s, int C, int blocks, const float* da, const float* z, const float* mean, const float* invstd, const float* g, const float* be,
                         const uint8_t* keep, float scale, int n, int h, int w, double* partial, int creal = 0);
// returns its grid (at most max_blocks): the workgroups whose column sums `partial` then holds
int tany_bn_bwd(hipStream_t s, int C, int max_blocks, const float* da, float* z, const float* mean, const float* invstd, const float* g, const float* be,
                const uint8_t* keep, float scale, const float* sums, float inv_count, int n, int h, int w, double* partial, int creal = 0);

// fc1 at P positions: hpart [P][n][100] partial planes, hsum [n][100] = their sum in position order (null: no sum and no launch for it -- the
// 80x80 head adds the planes itself)
void tany_fc1(hipStream_t s, const TrainAnyGeom& g, int n, const float* a3, const float* w, float* hpart, float* hsum);
void tany_fc1_wgrad(hipStream_t s, const TrainAnyGeom& g, int n, const float* a3, const float* dh, float* gw);
void tany_fc1_dgrad(hipStream_t s, const TrainAnyGeom& g, int n, const float* dh, const float* w, float* da3);

}  // namespace trexhip
