// cnn_weights.h -- the identity network's weight blob and the operand images the kernels read: host code only, no device call.
// cnn.hip (trexhip_load_weights) and train.hip (the trainer's import / export) parse the blob here; cnn.hip uploads what the
// packers return.  Every packer is a pure function of host floats, so its bytes are pinned by a CPU test (tests/test_cnn_weights.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace trexhip {

void set_error(const std::string& msg);        // capi.hip

// The blob (trex_amd/weights.py): 8 x int32 header {magic 'TRXW', version 1, classes, W, H, CH, architecture id, 0}, then (id 0, V118_3) these float32 tensors
// in PyTorch's state_dict order and shapes.  The six tensors of a convolution layer are consecutive: weight, bias, BN gamma, beta,
// running mean, running variance
enum { T_C1W, T_C1B, T_G1, T_BE1, T_RM1, T_RV1, T_C2W, T_C2B, T_G2, T_BE2, T_RM2, T_RV2, T_C3W, T_C3B, T_G3, T_BE3, T_RM3, T_RV3,
       T_F1W, T_F1B, T_LNG, T_LNB, T_F2W, T_F2B, T_COUNT };

size_t weight_tensor_count(int t, int classes, int CH, int W, int H);    // elements of tensor t
size_t weight_blob_bytes(int classes, int CH, int W, int H);             // header + all tensors
void write_weight_blob_header(void* blob, int classes, int W, int H, int CH);

struct WeightBlob { int classes, W, H, CH; const float* t[T_COUNT]; };   // the tensors point into the caller's blob
// Checks the header and the size; `who` prefixes the error texts.  `size_check`, when given, judges the individual_image_size between
// the magic and the channel check (each caller supports its own range) and returns TREXHIP_OK or the code it has set an error for.
// A blob of another architecture (header word 6 != 0) is refused here: TREXHIP_E_INVALID outside 0..4, else TREXHIP_E_UNSUPPORTED with a text that
// names the version -- trexhip_load_weights looks at the word first (blob_arch_id) and hands those blobs to parse_arch_blob.
int parse_weight_blob(const void* blob, size_t bytes, const char* who, WeightBlob* view, int (*size_check)(int W, int H) = nullptr);

// The fp16 operand images: w * 2^k in two pieces h1 = fp16(x), h2 = fp16(x - h1), k = floor(log2(16384 / max|w|)) clamped to +-24,
// so that max|w| * 2^k is in [8192, 16384).  The kernel multiplies its result by 2^-k
float pow2_scale(double max_abs, float* inv);                            // returns 2^k, *inv = 2^-k
void split_f16x2(float x, uint16_t out[2]);

struct Folded { std::vector<float> w, b; };                              // weights in a kernel's layout + their bias
struct ScaledImage { std::vector<uint16_t> v; float inv = 1.f; };        // fp16 pieces of w * 2^k, and 2^-k

// conv weight [CO][CI][5][5] + BN(eval) of `layer` (its six tensors) -> packed [CI/CIC][25][CIC][CO] (scaled) + bias[CO]
Folded fold_conv(const float* const* layer, int CO, int CI, int CIC);
// conv1: [16][CH][25] -> [CH][25][16] + bias[16] (chunks of one channel)
inline Folded fold_conv1(const float* const* layer, int CH) { return fold_conv(layer, 16, CH, 1); }
// packed fp32 conv weights [cc][25][CIC][CO] -> three bf16 pieces (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), round to
// nearest even) laid out [cc][tap][piece][k/8][co][8]
std::vector<uint16_t> pack_bf16x3(const std::vector<float>& wp, int CI, int CO, int CIC = 16);
// the same for the fp16 split: two pieces, [cc][tap][piece][k/8][co][8]
ScaledImage pack_f16x2(const std::vector<float>& wp, int CI, int CO, int CIC = 16);
// Winograd-domain weights of k_conv5_wino: Wt[ky][p] = sum_kx G[p][kx] w[ky][kx] (double), scaled by a power of two so that
// max|Wt| is in [8192, 16384), two fp16 pieces, laid out [cc][ky][p][piece][k-octet][co] x 8 halves
ScaledImage pack_wino_f16(const std::vector<float>& wp /*[cc][25][16][CO]*/, int CI, int CO);
// B fragments of the matrix-core conv1 (k_conv1_mfma: CH 1, k_conv1_mfma3: CH 3) from the folded [CH][25][16]:
// [shift s 0..3][mfma m 0..CH][piece hi|lo][lane] x 8 halves.  Lane = (q = lane / 16, co = lane % 16); slot j of its 8 halves is tap
// kx = j - s of one kernel row (zero outside 0..4).  MFMA m < CH holds channel m, rows ky = q; the last one holds row ky = 4 of channel q
// (zero for q >= CH)
ScaledImage pack_conv1_frags(const std::vector<float>& w1, int CH);
// fc1 [100][c*P + h*(W/8) + w] (the reference's NCHW flatten, P = (H/8)(W/8)) -> [(h*(W/8) + w)*128 + c][128 (o padded)], act3's NHWC
// order; bias padded to 128
Folded pack_fc1(const float* w, const float* b, int W, int H);
// the same matrix [K][128] as two fp16 pieces per weight, MFMA B-operand order [K/8][piece][128] x 8 halves
ScaledImage pack_fc1_f16(const std::vector<float>& wf);
// fc2 [classes][100] -> [100][classes]
std::vector<float> pack_fc2(const float* w, int classes);

// ---- v100, v110, v119, v200 (the layer table: cnn_arch_plan.h) ----
// header word 6 of a blob with the right magic and version; -1 otherwise
int blob_arch_id(const void* blob, size_t bytes);
size_t arch_blob_bytes(int id, int classes, int CH, int W, int H);      // 0 for an id, channel count or size no network has
// the tensors in the architecture's state_dict order, without num_batches_tracked: per convolution weight, bias and (with BatchNorm2d) gamma,
// beta, running mean, running variance; fc1, its BatchNorm1d where it has one, fc2
struct ArchBlob {
    int id, classes, W, H, CH;
    const float* conv[5][6];              // [layer][weight, bias, gamma, beta, mean, var]; the last four null without BatchNorm2d
    const float *fc1w, *fc1b, *bn1d[4], *fc2w, *fc2b;
};
int parse_arch_blob(const void* blob, size_t bytes, const char* who, ArchBlob* view);

// ---- the category network (trex_learn_category.py:18-44; the layer table: category_spec, cnn_arch_plan.h) ----
// Its blob (trex_amd/weights.py pack_category_blob): 8 x int32 header {magic 'TRXC', version 1, categories, W, H, CH, 0, 0}, then the float32 tensors
// in PyTorchModel's state_dict order: conv1.{weight,bias}, conv2.*, conv3.*, batch_norm1.{weight,bias,running_mean,running_var}, batch_norm2.*,
// batch_norm3.*, fc1.*, fc2.*.  The magic differs from an identity blob's, so each loader refuses the other's.
size_t category_blob_bytes(int categories, int CH, int W, int H);       // 0 outside 1..1024 categories, 1 or 3 channels, 8..256 each way
// view->id = ARCH_ID_CATEGORY, view->classes = categories, bn1d null.  A refusal names the field (size, magic, version, width, height, channels,
// categories) and `who`
int parse_category_blob(const void* blob, size_t bytes, const char* who, ArchBlob* view);
bool blob_is_category(const void* blob, size_t bytes);                  // its first word is the category magic (whatever else is wrong with it)
void write_category_blob_header(void* blob, int categories, int W, int H, int CH);

// One convolution for k_arch_conv: weight [CO][CI][T][T] -> fp32 [CO_pad/COB][CI_pad/16][T*T][16][COB] (zero where padded), and the epilogue's
// per-channel vectors relu((max_window(conv) * out_scale + bias) * s + t):  fold = true (v119, v200: BatchNorm in front of the pool) folds the
// BatchNorm into weights and bias in double, s = 1, t = 0;  fold = false keeps bias = the convolution's and s = gamma / sqrt(var + eps),
// t = beta - mean * s (v110: its scale may be negative behind a max-pool), or s = 1, t = 0 without BatchNorm (v100).  Padded channels: 0, 0, 0.
struct ArchConvImage { std::vector<float> w, bias, s, t; };
ArchConvImage pack_arch_conv(const float* const* layer, int CO, int CI, int taps, int CO_pad, int CI_pad, int COB, bool fold);
// the first layer for k_arch_conv1: [CO][CH][T][T] -> [CO_pad/16][CH][T*T][16]
ArchConvImage pack_arch_conv1(const float* const* layer, int CO, int CH, int taps, int CO_pad, bool fold);
// the pieces of such an image, [tile = (block, chunk, tap)][piece][k/8][co][8] as pack_bf16x3 / pack_f16x2 lay them out per tap
std::vector<uint16_t> pack_arch_bf16x3(const std::vector<float>& wp, int COB);
ScaledImage pack_arch_f16x2(const std::vector<float>& wp, int COB);
// fc1 [hidden][c*P + hw] (the reference's NCHW flatten of C channels at P positions; P = 1 behind the global average pool) ->
// [hw*C_pad + c][NH] in the activations' NHWC order (zero rows for padded channels, zero columns past `hidden`) + bias[NH]
Folded pack_arch_fc1(const float* w, const float* b, int hidden, int NH, int C, int C_pad, int P);
// the head's affine behind fc1: BatchNorm1d (bn = gamma, beta, mean, var) as s = gamma / sqrt(var + eps), t = beta - mean * s, or (bn null) 1, 0;
// Folded::w = s, Folded::b = t, both [NH], zero past `hidden`
Folded pack_arch_bn1d(const float* const* bn, int hidden, int NH);
// fc2 [classes][hidden] -> [hidden][classes]
std::vector<float> pack_arch_fc2(const float* w, int classes, int hidden);

}  // namespace trexhip
