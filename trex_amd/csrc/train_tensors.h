// train_tensors.h -- the tensors of the four networks that train (V118_3, v100, v110, the category network) as a trainer holds them, as one pure
// function of (network, W, H, CH, classes): the slots, torch's element counts, the counts held (padded), the offsets inside the four flat arrays
// P / G / M / V, the state_dict order, the map from torch's layout to the kernels', the dropout-mask planes of one sample and the slots Adam leaves
// alone.  No device code and no HIP: both trainers, trexhip_trainer_read and trexhip_trainer_export use this table and nothing else, and
// tests/cpp/print_train_tensors.cpp prints it for tests/test_train_tensors.py.
#pragma once
#include <stddef.h>
#include <initializer_list>

namespace trexhip {

enum TrainNet { TRAIN_V118_3, TRAIN_V100, TRAIN_V110, TRAIN_CATEGORY };

// Slots: six per convolution block (weight, bias, BatchNorm2d gamma, beta, running mean, running variance), then the head's.  A slot the network
// does not have holds nothing (count 0) and takes no room.  V118_3 numbers its 24 slots as its blob does (cnn_weights.h: T_*): the same up to the
// head's affine (S_G4, S_BE4 = its LayerNorm), then fc2 at 22 and 23
enum { K_W, K_B, K_G, K_BE, K_RM, K_RV };
enum { S_F1W = 18, S_F1B, S_G4, S_BE4, S_RM4, S_RV4, S_F2W, S_F2B, S_COUNT };
constexpr int TT_HID = 100;                  // fc1 outputs

struct TrainTensors {
    int CH, taps, c3;                        // input channels; taps x taps convolutions; block 3's real channels (travelling as 128)
    size_t P;                                // fc1's positions (H / 8)(W / 8), by successive floors
    int n_slots, n_tensors;
    int order[S_COUNT];                      // position in the state_dict (without num_batches_tracked) -> slot
    size_t off[S_COUNT + 1], cnt[S_COUNT], isz[S_COUNT];      // offset (a multiple of 64 floats), torch's element count, elements held
    size_t total;
    size_t keep_off[4], keep_row;            // dropout masks of one step: plane i of a batch of n starts at n * keep_off[i]; keep_row bytes per sample
    int buffers[8], n_buffers;               // running means and variances: Adam leaves them alone

    // index inside the slot, in the kernels' layout, of element `i` of torch's tensor: conv1 [c][tap][16], conv2 [tap][16][64], conv3
    // [ci / 32][tap][32][128], fc1 [hw][128][100] from torch's NCHW flatten over the c3 real channels; everything else as torch has it
    size_t to_internal(const int slot, const size_t i) const {
        const size_t T2 = (size_t)taps * taps;
        switch (slot) {
            case 0: { const size_t tap = i % T2, c = (i / T2) % CH, co = i / (T2 * CH); return (c * T2 + tap) * 16 + co; }
            case 6: { const size_t tap = i % T2, ci = (i / T2) % 16, co = i / (T2 * 16); return (tap * 16 + ci) * 64 + co; }
            case 12: { const size_t tap = i % T2, ci = (i / T2) % 64, co = i / (T2 * 64); return (((ci / 32) * T2 + tap) * 32 + ci % 32) * 128 + co; }
            case S_F1W: { const size_t K = c3 * P, k = i % K, o = i / K, c = k / P, hw = k % P; return (hw * 128 + c) * TT_HID + o; }
            default: return i;
        }
    }
};

inline TrainTensors train_tensors(const TrainNet net, const int W, const int H, const int CH, const int classes) {
    TrainTensors t{};
    const bool v118 = net == TRAIN_V118_3, cat = net == TRAIN_CATEGORY;
    const bool bn2d = net != TRAIN_V100, bn1d = net == TRAIN_V110;
    t.CH = CH; t.taps = cat ? 3 : 5; t.c3 = v118 ? 128 : 100;
    t.P = (size_t)(H / 8) * (W / 8);
    const size_t T2 = (size_t)t.taps * t.taps;
    const int CR[3] = {16, 64, t.c3}, CP[3] = {16, 64, 128};
    for (int i = 0; i < 3; ++i) {
        const size_t ci_r = i ? CR[i - 1] : CH, ci_p = i ? CP[i - 1] : CH;
        t.cnt[6 * i] = CR[i] * ci_r * T2; t.isz[6 * i] = CP[i] * ci_p * T2;
        for (int k = K_B; k <= K_RV; ++k)
            if (k == K_B || bn2d) { t.cnt[6 * i + k] = CR[i]; t.isz[6 * i + k] = CP[i]; }
    }
    const int f2w = v118 ? S_RM4 : S_F2W;    // V118_3 has no slot between its LayerNorm and fc2
    t.n_slots = f2w + 2;
    t.cnt[S_F1W] = (size_t)TT_HID * t.c3 * t.P; t.isz[S_F1W] = t.P * 128 * TT_HID;
    t.cnt[S_F1B] = t.isz[S_F1B] = TT_HID;
    for (int k = S_G4; k <= (bn1d ? S_RV4 : v118 ? S_BE4 : S_F1B); ++k) t.cnt[k] = t.isz[k] = TT_HID;
    t.cnt[f2w] = t.isz[f2w] = (size_t)classes * TT_HID; t.cnt[f2w + 1] = t.isz[f2w + 1] = classes;
    for (int k = 0; k < t.n_slots; ++k) { t.off[k] = t.total; t.total += (t.isz[k] + 63) / 64 * 64; }
    for (int k = t.n_slots; k <= S_COUNT; ++k) t.off[k] = t.total;
    // the state_dict: the slots in ascending order, but the category network declares its three convolutions ahead of its three BatchNorm2d
    if (cat)
        for (int k : {0, 1, 6, 7, 12, 13}) t.order[t.n_tensors++] = k;
    for (int k = 0; k < t.n_slots; ++k)
        if (t.cnt[k] && !(cat && k < 18 && k % 6 < K_G)) t.order[t.n_tensors++] = k;
    for (int k = 0; k < t.n_slots; ++k)
        if (t.cnt[k] && (k < 18 ? k % 6 >= K_RM : bn1d && k >= S_RM4 && k <= S_RV4)) t.buffers[t.n_buffers++] = k;
    // the mask planes: a byte per channel behind each block (Dropout2d), or, the category network, per pooled element of its real channels
    // (nn.Dropout); then a byte per fc1 output
    int h = H, w = W;
    for (int i = 0; i < 3; ++i) {
        h /= 2; w /= 2;
        t.keep_off[i] = t.keep_row;
        t.keep_row += cat ? (size_t)h * w * CR[i] : (size_t)CR[i];
    }
    t.keep_off[3] = t.keep_row; t.keep_row += TT_HID;
    return t;
}

}  // namespace trexhip
