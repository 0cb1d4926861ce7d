// cnn_weights.hip -- weight blob -> folded / repacked operand images of the identity network (cnn_weights.h).  Host code only; it is
// a .hip file for _Float16, whose conversions are the fp16 rounding of the images.
#include "cnn_weights.h"
#include "../../include/trexhip.h"
#include <cmath>
#include <cstring>

namespace trexhip {

// ---- the blob ----
static constexpr int32_t BLOB_MAGIC = 0x57585254, BLOB_VERSION = 1;      // 'TRXW'
size_t weight_tensor_count(int t, int classes, int CH, int W, int H) {
    switch (t) {
        case T_C1W: return (size_t)16 * CH * 25;
        case T_C1B: case T_G1: case T_BE1: case T_RM1: case T_RV1: return 16;
        case T_C2W: return (size_t)64 * 16 * 25;
        case T_C2B: case T_G2: case T_BE2: case T_RM2: case T_RV2: return 64;
        case T_C3W: return (size_t)128 * 64 * 25;
        case T_C3B: case T_G3: case T_BE3: case T_RM3: case T_RV3: return 128;
        case T_F1W: return (size_t)100 * 128 * (W / 8) * (H / 8);
        case T_F1B: case T_LNG: case T_LNB: return 100;
        case T_F2W: return (size_t)classes * 100;
        case T_F2B: return classes;
    }
    return 0;
}

size_t weight_blob_bytes(int classes, int CH, int W, int H) {
    size_t n = 0;
    for (int k = 0; k < T_COUNT; ++k) n += weight_tensor_count(k, classes, CH, W, H);
    return 32 + 4 * n;
}

void write_weight_blob_header(void* blob, int classes, int W, int H, int CH) {
    const int32_t hdr[8] = {BLOB_MAGIC, BLOB_VERSION, classes, W, H, CH, 0, 0};
    std::memcpy(blob, hdr, 32);
}

int parse_weight_blob(const void* blob, size_t bytes, const char* who, WeightBlob* view, int (*size_check)(int W, int H)) {
    const std::string pre = std::string(who) + ": ";
    if (bytes < 32) { set_error(pre + "blob too small"); return TREXHIP_E_INVALID; }
    int32_t hdr[8];
    std::memcpy(hdr, blob, 32);
    if (hdr[0] != BLOB_MAGIC || hdr[1] != BLOB_VERSION) { set_error(pre + "bad magic/version"); return TREXHIP_E_INVALID; }
    const int classes = hdr[2], W = hdr[3], H = hdr[4], CH = hdr[5];
    if (size_check) { const int rc = size_check(W, H); if (rc != TREXHIP_OK) return rc; }
    if (CH != 1 && CH != 3) { set_error(pre + "channels must be 1 or 3"); return TREXHIP_E_UNSUPPORTED; }
    if (classes < 1 || classes > 1024) { set_error(pre + "classes must be 1..1024"); return TREXHIP_E_INVALID; }
    if (bytes != weight_blob_bytes(classes, CH, W, H)) { set_error(pre + "blob size does not match its header"); return TREXHIP_E_INVALID; }
    view->classes = classes; view->W = W; view->H = H; view->CH = CH;
    const float* p = reinterpret_cast<const float*>(static_cast<const char*>(blob) + 32);
    for (int k = 0; k < T_COUNT; ++k) { view->t[k] = p; p += weight_tensor_count(k, classes, CH, W, H); }
    return TREXHIP_OK;
}

// ---- scale and pieces ----
float pow2_scale(double max_abs, float* inv) {
    int k = 0;
    if (max_abs > 0.0) { k = (int)std::floor(std::log2(16384.0 / max_abs)); if (k > 24) k = 24; if (k < -24) k = -24; }
    *inv = std::ldexp(1.0f, -k);
    return std::ldexp(1.0f, k);
}

void split_f16x2(float x, uint16_t out[2]) {
    const _Float16 h1 = (_Float16)x;
    const _Float16 h2 = (_Float16)(x - (float)h1);
    std::memcpy(&out[0], &h1, 2); std::memcpy(&out[1], &h2, 2);
}

static void split_bf16x3(float x, uint16_t out[3]) {      // piece = bf16 of what is left, round to nearest even
    for (int s = 0; s < 3; ++s) {
        uint32_t u; std::memcpy(&u, &x, 4);
        u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
        out[s] = (uint16_t)(u >> 16);
        float piece; std::memcpy(&piece, &u, 4);
        x -= piece;
    }
}

static float max_abs(const std::vector<float>& v) {
    float mx = 0.f;
    for (float x : v) mx = std::fmax(mx, std::fabs(x));
    return mx;
}

// element (cc, t, k, co) of a packed [ncc][T][CIC][CO] tensor -> its NP pieces (split(element index, pieces)) at [cc][t][piece][k/8][co][8]:
// the operand order of the 16-deep MFMAs, eight consecutive k of one output channel in one 16-byte load
template <int NP, class Split>
static std::vector<uint16_t> piece_image(int ncc, int T, int CIC, int CO, Split split) {
    const int KO = CIC / 8;
    std::vector<uint16_t> o((size_t)ncc * T * NP * KO * CO * 8);
    for (int cc = 0; cc < ncc; ++cc)
        for (int t = 0; t < T; ++t)
            for (int k = 0; k < CIC; ++k)
                for (int co = 0; co < CO; ++co) {
                    uint16_t pc[NP];
                    split((((size_t)cc * T + t) * CIC + k) * CO + co, pc);
                    for (int s = 0; s < NP; ++s) o[(((((size_t)cc * T + t) * NP + s) * KO + k / 8) * CO + co) * 8 + (k & 7)] = pc[s];
                }
    return o;
}

// BatchNorm (eval) folded into the convolution in double: w' = w s, b' = (b - mean) s + beta, s = gamma / sqrt(var + eps)
Folded fold_conv(const float* const* layer, int CO, int CI, int CIC) {
    const float *w = layer[0], *b = layer[1], *g = layer[2], *beta = layer[3], *mean = layer[4], *var = layer[5];
    Folded f{std::vector<float>((size_t)CO * CI * 25, 0.f), std::vector<float>(CO, 0.f)};
    for (int co = 0; co < CO; ++co) {
        const double s = (double)g[co] / std::sqrt((double)var[co] + 1e-5);     // BatchNorm2d eps
        f.b[co] = (float)(((double)b[co] - (double)mean[co]) * s + (double)beta[co]);
        for (int ci = 0; ci < CI; ++ci)
            for (int tap = 0; tap < 25; ++tap)
                f.w[((((size_t)(ci / CIC)) * 25 + tap) * CIC + ci % CIC) * CO + co] = (float)((double)w[((size_t)co * CI + ci) * 25 + tap] * s);
    }
    return f;
}

// ---- operand images ----
std::vector<uint16_t> pack_bf16x3(const std::vector<float>& wp, int CI, int CO, int CIC) {
    return piece_image<3>(CI / CIC, 25, CIC, CO, [&](size_t i, uint16_t* pc) { split_bf16x3(wp[i], pc); });
}

ScaledImage pack_f16x2(const std::vector<float>& wp, int CI, int CO, int CIC) {
    ScaledImage im;
    const float sc = pow2_scale(max_abs(wp), &im.inv);
    im.v = piece_image<2>(CI / CIC, 25, CIC, CO, [&](size_t i, uint16_t* pc) { split_f16x2(wp[i] * sc, pc); });
    return im;
}

ScaledImage pack_wino_f16(const std::vector<float>& wp, int CI, int CO) {
    static const double Gm[8][5] = {{-1, 0, 0, 0, 0},
                                    {-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9},
                                    {-2.0 / 9, 2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9},
                                    {1.0 / 90, 1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45},
                                    {1.0 / 90, -1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45},
                                    {32.0 / 45, 16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45},
                                    {32.0 / 45, -16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45},
                                    {0, 0, 0, 0, 1}};
    const int ncc = CI / 16;
    std::vector<double> wt((size_t)ncc * 40 * 16 * CO);                  // [cc][ky * 8 + p][16][CO]
    double mx = 0.0;
    for (int cc = 0; cc < ncc; ++cc)
        for (int ky = 0; ky < 5; ++ky)
            for (int p = 0; p < 8; ++p)
                for (int kk = 0; kk < 16; ++kk)
                    for (int co = 0; co < CO; ++co) {
                        double a = 0.0;
                        for (int kx = 0; kx < 5; ++kx) a += Gm[p][kx] * (double)wp[(((size_t)cc * 25 + ky * 5 + kx) * 16 + kk) * CO + co];
                        wt[(((size_t)cc * 40 + ky * 8 + p) * 16 + kk) * CO + co] = a;
                        mx = std::fmax(mx, std::fabs(a));
                    }
    ScaledImage im;
    const double sc = pow2_scale(mx, &im.inv);
    im.v = piece_image<2>(ncc, 40, 16, CO, [&](size_t i, uint16_t* pc) { split_f16x2((float)(wt[i] * sc), pc); });
    return im;
}

ScaledImage pack_conv1_frags(const std::vector<float>& w1, int CH) {
    ScaledImage im;
    const float sc = pow2_scale(max_abs(w1), &im.inv);
    const int NM = CH + 1;
    im.v.assign((size_t)4 * NM * 2 * 64 * 8, 0);
    for (int s = 0; s < 4; ++s)
        for (int m = 0; m < NM; ++m)
            for (int lane = 0; lane < 64; ++lane) {
                const int co = lane & 15, q = lane >> 4;
                const int ch = m < CH ? m : q, ky = m < CH ? q : 4;
                for (int slot = 0; slot < 8; ++slot) {
                    const int kx = slot - s;
                    float x = 0.f;
                    if (ch < CH && kx >= 0 && kx < 5) x = w1[((size_t)ch * 25 + ky * 5 + kx) * 16 + co] * sc;
                    uint16_t pc[2];
                    split_f16x2(x, pc);
                    for (int piece = 0; piece < 2; ++piece) im.v[((size_t)((s * NM + m) * 2 + piece) * 64 + lane) * 8 + slot] = pc[piece];
                }
            }
    return im;
}

Folded pack_fc1(const float* w, const float* b, int W, int H) {
    const int P = (W / 8) * (H / 8);
    const size_t flat = (size_t)128 * P;
    Folded f{std::vector<float>(flat * 128, 0.f), std::vector<float>(128, 0.f)};
    for (int o = 0; o < 100; ++o) {
        f.b[o] = b[o];
        for (int c = 0; c < 128; ++c)
            for (int hw = 0; hw < P; ++hw) f.w[((size_t)hw * 128 + c) * 128 + o] = w[(size_t)o * flat + (size_t)c * P + hw];
    }
    return f;
}

ScaledImage pack_fc1_f16(const std::vector<float>& wf) {
    ScaledImage im;
    const float sc = pow2_scale(max_abs(wf), &im.inv);
    im.v = piece_image<2>((int)(wf.size() / 128 / 8), 1, 8, 128, [&](size_t i, uint16_t* pc) { split_f16x2(wf[i] * sc, pc); });
    return im;
}

std::vector<float> pack_fc2(const float* w, int classes) {
    std::vector<float> t((size_t)100 * classes);
    for (int c = 0; c < classes; ++c)
        for (int k = 0; k < 100; ++k) t[(size_t)k * classes + c] = w[(size_t)c * 100 + k];
    return t;
}

}  // namespace trexhip
