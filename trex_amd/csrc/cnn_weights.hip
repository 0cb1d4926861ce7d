// cnn_weights.hip -- weight blob -> folded / repacked operand images of the identity network (cnn_weights.h).  Host code only; it is
// a .hip file for _Float16, whose conversions are the fp16 rounding of the images.
#include "cnn_weights.h"
#include "cnn_arch_plan.h"
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
    if (hdr[6] < TREXHIP_NET_V118_3 || hdr[6] > TREXHIP_NET_V200) { set_error(pre + "unknown network version id " + std::to_string(hdr[6]) + " (0..4: v118_3, v100, v110, v119, v200)"); return TREXHIP_E_INVALID; }
    if (hdr[6] != TREXHIP_NET_V118_3) { set_error(pre + "the blob holds a " + arch_name(hdr[6]) + " network; only v118_3 is implemented here"); return TREXHIP_E_UNSUPPORTED; }
    if (size_check) { const int rc = size_check(W, H); if (rc != TREXHIP_OK) return rc; }
    if (CH != 1 && CH != 3) { set_error(pre + "channels must be 1 or 3"); return TREXHIP_E_UNSUPPORTED; }
    if (classes < 1 || classes > 1024) { set_error(pre + "classes must be 1..1024"); return TREXHIP_E_INVALID; }
    if (bytes != weight_blob_bytes(classes, CH, W, H)) { set_error(pre + "blob size does not match its header"); return TREXHIP_E_INVALID; }
    view->classes = classes; view->W = W; view->H = H; view->CH = CH;
    const float* p = reinterpret_cast<const float*>(static_cast<const char*>(blob) + 32);
    for (int k = 0; k < T_COUNT; ++k) { view->t[k] = p; p += weight_tensor_count(k, classes, CH, W, H); }
    return TREXHIP_OK;
}

// ---- the blobs of the other architectures ----
int blob_arch_id(const void* blob, size_t bytes) {
    if (bytes < 32) return -1;
    int32_t hdr[8];
    std::memcpy(hdr, blob, 32);
    return hdr[0] == BLOB_MAGIC && hdr[1] == BLOB_VERSION ? hdr[6] : -1;
}

// walks the tensors of (id, classes, CH, W, H) in blob order: f(elements) is called once per tensor and returns where it lies
template <class F>
static void arch_walk(const ArchSpec& s, int classes, int CH, int W, int H, ArchBlob* v, F next) {
    int ci = CH, h = H, w = W;
    for (int i = 0; i < s.n_conv; ++i) {
        const ArchConv& c = s.conv[i];
        const float* p = next((size_t)c.CO * ci * c.taps * c.taps);
        if (v) v->conv[i][0] = p;
        p = next(c.CO);
        if (v) v->conv[i][1] = p;
        for (int k = 2; k < 6; ++k) { p = s.bn2d ? next(c.CO) : nullptr; if (v) v->conv[i][k] = p; }
        ci = c.CO;
        if (c.pool) { h /= c.pool; w /= c.pool; }
    }
    const size_t flat = s.gap ? (size_t)ci : (size_t)ci * h * w;
    const float* p = next((size_t)s.hidden * flat);
    if (v) v->fc1w = p;
    p = next(s.hidden);
    if (v) v->fc1b = p;
    for (int k = 0; k < 4; ++k) { p = s.bn1d ? next(s.hidden) : nullptr; if (v) v->bn1d[k] = p; }
    p = next((size_t)classes * s.hidden);
    if (v) v->fc2w = p;
    p = next(classes);
    if (v) v->fc2b = p;
}

size_t arch_blob_bytes(int id, int classes, int CH, int W, int H) {
    if (id == TREXHIP_NET_V118_3) return (CH == 1 || CH == 3) && W >= 8 && W <= 256 && H >= 8 && H <= 256 && classes >= 1 && classes <= 1024 ? weight_blob_bytes(classes, CH, W, H) : 0;
    const ArchSpec* s = arch_spec(id);
    if (!s || (CH != 1 && CH != 3) || W < s->min_size || W > 256 || H < s->min_size || H > 256 || classes < 1 || classes > 1024) return 0;
    size_t n = 0;
    arch_walk(*s, classes, CH, W, H, nullptr, [&](size_t cnt) -> const float* { n += cnt; return nullptr; });
    return 32 + 4 * n;
}

int parse_arch_blob(const void* blob, size_t bytes, const char* who, ArchBlob* view) {
    const std::string pre = std::string(who) + ": ";
    if (bytes < 32) { set_error(pre + "blob too small"); return TREXHIP_E_INVALID; }
    int32_t hdr[8];
    std::memcpy(hdr, blob, 32);
    if (hdr[0] != BLOB_MAGIC || hdr[1] != BLOB_VERSION) { set_error(pre + "bad magic/version"); return TREXHIP_E_INVALID; }
    const int classes = hdr[2], W = hdr[3], H = hdr[4], CH = hdr[5], id = hdr[6];
    const ArchSpec* s = arch_spec(id);
    if (!s) { set_error(pre + "unknown network version id " + std::to_string(id) + " (0..4: v118_3, v100, v110, v119, v200)"); return TREXHIP_E_INVALID; }
    if (W < s->min_size || W > 256 || H < s->min_size || H > 256) {
        set_error(pre + "individual_image_size " + std::to_string(W) + "x" + std::to_string(H) + " is outside " + std::to_string(s->min_size) + "..256 x " +
                  std::to_string(s->min_size) + "..256, the range of " + s->name + " (minimum " + std::to_string(s->min_size) + ")");
        return TREXHIP_E_UNSUPPORTED;
    }
    if (CH != 1 && CH != 3) { set_error(pre + "channels must be 1 or 3"); return TREXHIP_E_UNSUPPORTED; }
    if (classes < 1 || classes > 1024) { set_error(pre + "classes must be 1..1024"); return TREXHIP_E_INVALID; }
    if (bytes != arch_blob_bytes(id, classes, CH, W, H)) { set_error(pre + "blob size does not match its header (" + s->name + ")"); return TREXHIP_E_INVALID; }
    view->id = id; view->classes = classes; view->W = W; view->H = H; view->CH = CH;
    const float* p = reinterpret_cast<const float*>(static_cast<const char*>(blob) + 32);
    arch_walk(*s, classes, CH, W, H, view, [&](size_t cnt) -> const float* { const float* at = p; p += cnt; return at; });
    return TREXHIP_OK;
}

// ---- the category network's blob ----
static constexpr int32_t CAT_MAGIC = 0x43585254;      // 'TRXC'
template <class F>
static void category_walk(int categories, int CH, int W, int H, ArchBlob* v, F next) {
    const ArchSpec& s = *category_spec();
    int ci = CH;
    for (int i = 0; i < s.n_conv; ++i) {
        const ArchConv& c = s.conv[i];
        const float* p = next((size_t)c.CO * ci * c.taps * c.taps);
        if (v) v->conv[i][0] = p;
        p = next(c.CO);
        if (v) v->conv[i][1] = p;
        ci = c.CO;
    }
    for (int i = 0; i < s.n_conv; ++i)
        for (int k = 2; k < 6; ++k) { const float* p = next(s.conv[i].CO); if (v) v->conv[i][k] = p; }
    const float* p = next((size_t)s.hidden * ci * (H / 8) * (W / 8));
    if (v) v->fc1w = p;
    p = next(s.hidden);
    if (v) v->fc1b = p;
    p = next((size_t)categories * s.hidden);
    if (v) v->fc2w = p;
    p = next(categories);
    if (v) v->fc2b = p;
}

size_t category_blob_bytes(int categories, int CH, int W, int H) {
    if ((CH != 1 && CH != 3) || W < 8 || W > 256 || H < 8 || H > 256 || categories < 1 || categories > 1024) return 0;
    size_t n = 0;
    category_walk(categories, CH, W, H, nullptr, [&](size_t cnt) -> const float* { n += cnt; return nullptr; });
    return 32 + 4 * n;
}

bool blob_is_category(const void* blob, size_t bytes) {
    int32_t magic = 0;
    if (bytes >= 4) std::memcpy(&magic, blob, 4);
    return magic == CAT_MAGIC;
}

void write_category_blob_header(void* blob, int categories, int W, int H, int CH) {
    const int32_t hdr[8] = {CAT_MAGIC, 1, categories, W, H, CH, 0, 0};
    std::memcpy(blob, hdr, 32);
}

int parse_category_blob(const void* blob, size_t bytes, const char* who, ArchBlob* view) {
    const std::string pre = std::string(who) + ": ";
    if (bytes < 32) { set_error(pre + "size: " + std::to_string(bytes) + " bytes are less than the header"); return TREXHIP_E_INVALID; }
    int32_t hdr[8];
    std::memcpy(hdr, blob, 32);
    if (hdr[0] != CAT_MAGIC) { set_error(pre + "magic: not a category blob ('TRXC')" + (hdr[0] == BLOB_MAGIC ? "; this is an identity blob ('TRXW', trexhip_load_weights)" : "")); return TREXHIP_E_INVALID; }
    if (hdr[1] != 1) { set_error(pre + "version: " + std::to_string(hdr[1]) + ", only 1 is known"); return TREXHIP_E_INVALID; }
    const int categories = hdr[2], W = hdr[3], H = hdr[4], CH = hdr[5];
    if (W < 8 || W > 256) { set_error(pre + "width: " + std::to_string(W) + " is outside 8..256"); return TREXHIP_E_UNSUPPORTED; }
    if (H < 8 || H > 256) { set_error(pre + "height: " + std::to_string(H) + " is outside 8..256"); return TREXHIP_E_UNSUPPORTED; }
    if (CH != 1 && CH != 3) { set_error(pre + "channels: " + std::to_string(CH) + ", must be 1 or 3"); return TREXHIP_E_UNSUPPORTED; }
    if (categories < 1 || categories > 1024) { set_error(pre + "categories: " + std::to_string(categories) + " is outside 1..1024"); return TREXHIP_E_INVALID; }
    const size_t want = category_blob_bytes(categories, CH, W, H);
    if (bytes != want) { set_error(pre + "size: " + std::to_string(bytes) + " bytes, the header asks for " + std::to_string(want)); return TREXHIP_E_INVALID; }
    *view = ArchBlob{};
    view->id = ARCH_ID_CATEGORY; view->classes = categories; view->W = W; view->H = H; view->CH = CH;
    const float* p = reinterpret_cast<const float*>(static_cast<const char*>(blob) + 32);
    category_walk(categories, CH, W, H, view, [&](size_t cnt) -> const float* { const float* at = p; p += cnt; return at; });
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

// ---- operand images of the other architectures ----
// the epilogue's vectors of one layer (see cnn_weights.h); returns the per-channel factor folded into the weights
static std::vector<double> arch_affine(const float* const* layer, int CO, int CO_pad, bool fold, ArchConvImage* im) {
    const float *b = layer[1], *g = layer[2], *beta = layer[3], *mean = layer[4], *var = layer[5];
    im->bias.assign(CO_pad, 0.f); im->s.assign(CO_pad, 0.f); im->t.assign(CO_pad, 0.f);
    std::vector<double> f(CO, 1.0);
    for (int co = 0; co < CO; ++co) {
        const double s = g ? (double)g[co] / std::sqrt((double)var[co] + 1e-5) : 1.0;     // BatchNorm2d eps
        if (fold) {
            f[co] = s;
            im->bias[co] = (float)(((double)b[co] - (double)mean[co]) * s + (double)beta[co]);
            im->s[co] = 1.f;
        } else {
            im->bias[co] = b[co];
            im->s[co] = (float)s;
            im->t[co] = g ? (float)((double)beta[co] - (double)mean[co] * s) : 0.f;
        }
    }
    return f;
}

ArchConvImage pack_arch_conv(const float* const* layer, int CO, int CI, int taps, int CO_pad, int CI_pad, int COB, bool fold) {
    ArchConvImage im;
    const std::vector<double> f = arch_affine(layer, CO, CO_pad, fold, &im);
    const int T2 = taps * taps, ncc = CI_pad / 16;
    im.w.assign((size_t)CO_pad * CI_pad * T2, 0.f);
    for (int co = 0; co < CO; ++co)
        for (int ci = 0; ci < CI; ++ci)
            for (int tap = 0; tap < T2; ++tap)
                im.w[(((((size_t)(co / COB)) * ncc + ci / 16) * T2 + tap) * 16 + ci % 16) * COB + co % COB] = (float)((double)layer[0][((size_t)co * CI + ci) * T2 + tap] * f[co]);
    return im;
}

ArchConvImage pack_arch_conv1(const float* const* layer, int CO, int CH, int taps, int CO_pad, bool fold) {
    ArchConvImage im;
    const std::vector<double> f = arch_affine(layer, CO, CO_pad, fold, &im);
    const int T2 = taps * taps;
    im.w.assign((size_t)CO_pad * CH * T2, 0.f);
    for (int co = 0; co < CO; ++co)
        for (int c = 0; c < CH; ++c)
            for (int tap = 0; tap < T2; ++tap)
                im.w[((((size_t)(co / 16)) * CH + c) * T2 + tap) * 16 + co % 16] = (float)((double)layer[0][((size_t)co * CH + c) * T2 + tap] * f[co]);
    return im;
}

std::vector<uint16_t> pack_arch_bf16x3(const std::vector<float>& wp, int COB) {
    return piece_image<3>((int)(wp.size() / ((size_t)16 * COB)), 1, 16, COB, [&](size_t i, uint16_t* pc) { split_bf16x3(wp[i], pc); });
}

ScaledImage pack_arch_f16x2(const std::vector<float>& wp, int COB) {
    ScaledImage im;
    const float sc = pow2_scale(max_abs(wp), &im.inv);
    im.v = piece_image<2>((int)(wp.size() / ((size_t)16 * COB)), 1, 16, COB, [&](size_t i, uint16_t* pc) { split_f16x2(wp[i] * sc, pc); });
    return im;
}

Folded pack_arch_fc1(const float* w, const float* b, int hidden, int NH, int C, int C_pad, int P) {
    const size_t flat = (size_t)C * P;
    Folded f{std::vector<float>((size_t)C_pad * P * NH, 0.f), std::vector<float>(NH, 0.f)};
    for (int o = 0; o < hidden; ++o) {
        f.b[o] = b[o];
        for (int c = 0; c < C; ++c)
            for (int hw = 0; hw < P; ++hw) f.w[((size_t)hw * C_pad + c) * NH + o] = w[(size_t)o * flat + (size_t)c * P + hw];
    }
    return f;
}

Folded pack_arch_bn1d(const float* const* bn, int hidden, int NH) {
    Folded f{std::vector<float>(NH, 0.f), std::vector<float>(NH, 0.f)};
    for (int o = 0; o < hidden; ++o) {
        const double s = bn && bn[0] ? (double)bn[0][o] / std::sqrt((double)bn[3][o] + 1e-5) : 1.0;     // BatchNorm1d eps
        f.w[o] = (float)s;
        f.b[o] = bn && bn[0] ? (float)((double)bn[1][o] - (double)bn[2][o] * s) : 0.f;
    }
    return f;
}

std::vector<float> pack_arch_fc2(const float* w, int classes, int hidden) {
    std::vector<float> t((size_t)hidden * classes);
    for (int c = 0; c < classes; ++c)
        for (int k = 0; k < hidden; ++k) t[(size_t)k * classes + c] = w[(size_t)c * hidden + k];
    return t;
}

std::vector<float> pack_fc2(const float* w, int classes) {
    std::vector<float> t((size_t)100 * classes);
    for (int c = 0; c < classes; ++c)
        for (int k = 0; k < 100; ++k) t[(size_t)k * classes + c] = w[(size_t)c * 100 + k];
    return t;
}

}  // namespace trexhip
