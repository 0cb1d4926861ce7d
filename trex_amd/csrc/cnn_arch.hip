// cnn_arch.hip -- the identity networks v100, v110, v119 and v200 (visual_identification_network_torch.py:30-382; the layer table: cnn_arch_plan.h)
// at any individual_image_size of their range, inference only.  NHWC fp32 activations throughout, every pool floors like nn.MaxPool2d.
//
//   k_arch_conv1<CH, T>   first layer, u8 crops -> fp32, T x T taps, 16 output channels per workgroup (grid y = CO / 16), exact fp32 on the VALU
//   k_arch_conv<COB, ..>  every further convolution as T * T shifted GEMMs on the matrix cores: run-time CI, taps 3 or 5, fused floor 2x2 max-pool
//                         or none, COB = 32 / 64 / 128 output channels per workgroup with the channel block on the grid's y, the three
//                         arithmetic kinds, the fp16 range flag per crop and the guarded bf16x6 re-run
//                         -- both are the TiledArgs instances of the bodies in conv_tiled.h, which the any-size V118_3 chain (cnn_any.hip) shares
//   k_pool3               floor 3x3 max-pool, streaming, one float4 of channels per lane (v200: a 3x3 window does not fit the window-major tile)
//   k_gap                 global average pool (v200), summed in raster order
//   k_arch_fc1            fc1 as an exact fp32 GEMM on the matrix cores, K split over the 4 waves of a workgroup and summed in wave order
//   k_arch_head           BatchNorm1d or none + ReLU + fc2 + softmax, one wave per crop, the expressions of k_head (cnn.hip)
//   k_cat_label           the category network only: label = index of the first maximum of a crop's logits, one wave per crop, behind the head
//
// The category network (trex_learn_category.py:18-44; category_spec, cnn_arch_plan.h) runs the same chain from the context's second slot
// (ctx->cat): its first layer is the NORM instance of k_arch_conv1, which stages x / 127.5 - 1 instead of x, and k_cat_label follows its head.
//
// The epilogue of both convolution kernels puts the layer's affine (s, t) BEHIND the pool (conv_tiled.h): v110 needs it, v119 / v200 fold their
// BatchNorm into weights and bias (s = 1, t = 0), v100 has none.
//
// A call's crops are walked in chunks of ArchPlan::chunk (a constant of version and size); every kernel computes a crop from that crop alone, in
// an order that does not depend on the chunk or on n, so a crop's row is the same bits wherever it stands.
#include "cnn_arch.h"
#include "conv_tiled.h"
#include "cnn_weights.h"

namespace trexhip {
namespace {

// The first layer: conv1_tiled (conv_tiled.h) with CO, the pool and the affine as arguments and the block of 16 output channels on the grid's y.
// NORM: the category network's, which stages x / 127.5 - 1; the identity instances compile without it.
template <int CH, int T, bool NORM = false>
__global__ __launch_bounds__(256) void k_arch_conv1(const uint8_t* __restrict__ crops /*[N][H][W][CH]*/, const float* __restrict__ w /*[CO/16][CH][T*T][16]*/,
                                                    const float* __restrict__ bias, const float* __restrict__ sv, const float* __restrict__ tv,
                                                    float* __restrict__ out /*[N][Ho][Wo][CO]*/, const int CO, const int W, const int H, const int pool,
                                                    const int tx_n, const int tiles) {
    conv1_tiled<CH, T, NORM>(TiledArgs{CH, CO, T, pool, sv, tv}, crops, w, bias, out, W, H, tx_n, tiles);
}

// Every further convolution: conv_tiled (conv_tiled.h) with CI, CO, taps (3 or 5) and pool as arguments, COB = 32 / 64 / 128 output channels
// per workgroup on the grid's y, input channels staged 16 at a time.  wp: pack_arch_conv / pack_arch_bf16x3 / pack_arch_f16x2.
template <int COB, int KIND, int NTERMS>
__global__ __launch_bounds__(512) void k_arch_conv(const float* __restrict__ in /*[N][Hi][Wi][CI]*/, const uint4* __restrict__ wp, const float* __restrict__ bias,
                                                   const float* __restrict__ sv, const float* __restrict__ tv, float* __restrict__ out /*[N][Ho][Wo][CO]*/,
                                                   const int CI, const int CO, const int Hi, const int Wi, const int taps, const int pool, const int TX,
                                                   const int tx_n, const int tiles, const float out_scale, uint32_t* __restrict__ overflow,
                                                   uint8_t* __restrict__ crop_flags, const uint32_t* __restrict__ guard, const int n_blocks) {
    conv_tiled<COB, KIND, NTERMS, 16>(TiledArgs{CI, CO, taps, pool, sv, tv}, in, wp, bias, out, Hi, Wi, TX, tx_n, tiles, out_scale, overflow, crop_flags, guard,
                                      n_blocks);
}

// ------------------------------------------------------------------------------------------------
// floor 3x3 max-pool, NHWC, one float4 of channels per lane: reads the layer's output once and writes a ninth of it
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pool3(const float4* __restrict__ in /*[N][Hi][Wi][C4]*/, float4* __restrict__ out /*[N][Hi/3][Wi/3][C4]*/, const int n,
                                               const int Hi, const int Wi, const int C4, const uint32_t* __restrict__ guard) {
    if (guard && guard[1] == 0u) return;
    const int items = (guard && guard[1] == 1u) ? (int)guard[0] : n;
    const int Ho = Hi / 3, Wo = Wi / 3;
    const size_t total = (size_t)items * Ho * Wo * C4;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int c = (int)(idx % C4);
        size_t r = idx / C4;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int crop = plan_crop(guard, (int)(r / Ho));
        const float4* src = in + (((size_t)crop * Hi + 3 * oy) * Wi + 3 * ox) * C4 + c;
        float4 m = src[0];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float4 v = src[((size_t)dy * Wi + dx) * C4];
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        out[(((size_t)crop * Ho + oy) * Wo + ox) * C4 + c] = m;
    }
}

// global average pool: the P positions of a channel summed in raster order, then one division
__global__ __launch_bounds__(256) void k_gap(const float* __restrict__ in /*[N][P][C]*/, float* __restrict__ out /*[N][C]*/, const int n, const int P, const int C) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * C) return;
    const size_t crop = idx / C;
    const int c = (int)(idx - crop * C);
    const float* src = in + crop * P * C + c;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += src[(size_t)p * C];
    out[idx] = s / (float)P;
}

// ------------------------------------------------------------------------------------------------
// fc1: out[n][NH] = act[n][K] x w[K][NH] + bias, exact fp32 (v_mfma_f32_32x32x2_f32)
// ------------------------------------------------------------------------------------------------
// Grid (ceil(n / 32), NH / 32): 32 crops x 32 outputs per workgroup.  Wave v of the 4 walks the k-octets v, v + 4, ... (K is a multiple of 8);
// the four partial tiles meet in LDS (4 * 32 * 33 * 4 = 16896 B) and are summed in wave order.  The split is the layer's, never n's.
__global__ __launch_bounds__(256) void k_arch_fc1(const float* __restrict__ act /*[n][K]*/, const float* __restrict__ w /*[K][NH]*/, const float* __restrict__ bias,
                                                  float* __restrict__ out /*[n][NH]*/, const int n, const int K, const int NH) {
    __shared__ float red[4][32][33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * 32, col0 = blockIdx.y * 32;
    const int row = row0 + j < n ? row0 + j : n - 1;                    // rows past the batch repeat its last crop and are not written
    const float* a = act + (size_t)row * K + 4 * h;
    const float* b = w + (size_t)(4 * h) * NH + col0 + j;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int ko = wave; ko < K / 8; ko += 4) {
        const float4 av = *reinterpret_cast<const float4*>(a + (size_t)ko * 8);
        const float* bp = b + (size_t)ko * 8 * NH;
        const float b0 = bp[0], b1 = bp[NH], b2 = bp[2 * (size_t)NH], b3 = bp[3 * (size_t)NH];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b3, acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave][8 * g + 4 * h + q][j] = acc[4 * g + q];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int idx = tid + 256 * r, i = idx >> 5, c = idx & 31;
        if (row0 + i >= n) continue;
        out[(size_t)(row0 + i) * NH + col0 + c] = ((red[0][i][c] + red[1][i][c]) + red[2][i][c]) + red[3][i][c] + bias[col0 + c];
    }
}

// ------------------------------------------------------------------------------------------------
// head: (BatchNorm1d as s, t) + ReLU + fc2 + softmax, one wave per crop
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float arch_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float arch_wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(256) void k_arch_head(const float* __restrict__ fc1 /*[n][NH]*/, const float* __restrict__ hs, const float* __restrict__ ht,
                                                   const float* __restrict__ w2t /*[hidden][C]*/, const float* __restrict__ b2, float* __restrict__ probs /*[n][C]*/,
                                                   float* __restrict__ logits_out, const int n, const int C, const int NH, const int hidden) {
    __shared__ float ys[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int crop = blockIdx.x * 4 + wave;
    if (crop >= n) return;
    const float* x = fc1 + (size_t)crop * NH;
    for (int k = lane; k < NH; k += 64) ys[wave][k] = fmaxf(x[k] * hs[k] + ht[k], 0.f);
    __builtin_amdgcn_wave_barrier();      // ys[wave] is private to this wave; LDS ops of one wave stay in order
    const int nrep = (C + 63) / 64;
    float mx = -3.4e38f, sum = 0.f;
    float lg[16];                         // up to 1024 classes
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        lg[r] = -3.4e38f;
        if (r < nrep) {
            const int c = r * 64 + lane;
            if (c < C) {
                float s = b2[c];
                for (int k = 0; k < hidden; ++k) s = fmaf(ys[wave][k], w2t[(size_t)k * C + c], s);
                lg[r] = s;
                if (logits_out) logits_out[(size_t)crop * C + c] = s;
            }
            mx = fmaxf(mx, lg[r]);
        }
    }
    mx = arch_wave_max(mx);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < nrep) {
            const int c = r * 64 + lane;
            if (c < C) { lg[r] = expf(lg[r] - mx); sum += lg[r]; }
        }
    sum = 1.f / arch_wave_sum(sum);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (r < nrep) {
            const int c = r * 64 + lane;
            if (c < C) probs[(size_t)crop * C + c] = lg[r] * sum;
        }
}

// the category network's label (trex_learn_category.py:441, softmax(..).argmax(dim=1)): the index of the FIRST maximum of the crop's logits -- the
// softmax is monotonic, and its row is the head's.  One wave per crop: a lane keeps the first maximum of its columns lane, lane + 64, ..., the
// wave keeps the larger value and, between equal ones, the lower index.  Reads 4 C bytes per crop, writes 4.
__global__ __launch_bounds__(256) void k_cat_label(const float* __restrict__ logits /*[n][C]*/, int32_t* __restrict__ labels, const int n, const int C) {
    const int lane = threadIdx.x & 63, crop = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (crop >= n) return;
    const float* x = logits + (size_t)crop * C;
    float best = -INFINITY;
    int at = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const float v = x[c];
        if (at == 0x7fffffff || v > best) { best = v; at = c; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oa = __shfl_xor(at, d);
        if (oa != 0x7fffffff && (at == 0x7fffffff || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    if (lane == 0) labels[crop] = at;
}

// the plan of a chunk's guarded re-run (guard_plan, conv_tiled.h): lists the flagged crops, clears their flags and the range word, and adds what
// it planned to the call's two statistics words
__global__ __launch_bounds__(1024) void k_arch_guard_plan(uint32_t* __restrict__ overflow, uint8_t* __restrict__ flags, const int n, uint32_t* __restrict__ plan,
                                                          uint32_t* __restrict__ stats) {
    __shared__ uint32_t cnt;
    guard_plan<1024>(overflow, flags, n, plan, cnt, stats);
}

// ---- the instances, each stated once ----
using ArchKern = decltype(Kern(k_arch_conv<128, 2, 1>, 512));
template <int COB, int KIND, int NTERMS>
ArchKern arch_kern() { return Kern(k_arch_conv<COB, KIND, NTERMS>, 512, TileGeom<COB, KIND, 16>::LDS_BYTES); }
struct ArchConvSet { ArchKern by_mode[4]; };     // indexed by TREXHIP_CNN_*: FP32, BF16X6, BF16X3, FP16X3
template <int COB>
ArchConvSet arch_set() { return {{arch_kern<COB, 2, 1>(), arch_kern<COB, 0, 6>(), arch_kern<COB, 0, 3>(), arch_kern<COB, 1, 3>()}}; }
const ArchConvSet ARCH_CONV[3] = {arch_set<32>(), arch_set<64>(), arch_set<128>()};      // COB 32, 64, 128
const ByChannels ARCH_CONV1_T3{Kern(k_arch_conv1<1, 3>, 256), Kern(k_arch_conv1<3, 3>, 256)};
const ByChannels ARCH_CONV1_T3N{Kern(k_arch_conv1<1, 3, true>, 256), Kern(k_arch_conv1<3, 3, true>, 256)};      // the category network's
const Kern K_CAT_LABEL(k_cat_label, 256);
const ByChannels ARCH_CONV1_T5{Kern(k_arch_conv1<1, 5>, 256), Kern(k_arch_conv1<3, 5>, 256)};
const Kern K_POOL3(k_pool3, 256);
const Kern K_GAP(k_gap, 256);
const Kern K_ARCH_FC1(k_arch_fc1, 256);
const Kern K_ARCH_HEAD(k_arch_head, 256);
const Kern K_ARCH_GUARD_PLAN(k_arch_guard_plan, 1024);

inline int cdiv(const size_t a, const size_t b) { return (int)((a + b - 1) / b); }

// one convolution of the chain behind the first on m crops, or (guard) on the plan's
void launch_conv(hipStream_t s, const Net& net, const ArchNet& a, const int i, const int mode, const int m, const uint32_t* guard, const int n_cus) {
    const ArchLayerPlan& l = a.plan.L[i];
    const ArchLayerDev &d = a.L[i], &prev = a.L[i - 1];
    const bool h16 = mode == TREXHIP_CNN_FP16X3;
    const void* w = mode == TREXHIP_CNN_FP32 ? (const void*)d.w : h16 ? (const void*)d.wh : (const void*)d.ws;
    const int items = m * l.tl.tiles;
    const int gx = guard ? std::min(items, 4 * n_cus) : items;          // a re-run is a handful of crops: a small grid strides over them
    ARCH_CONV[l.COB == 32 ? 0 : l.COB == 64 ? 1 : 2].by_mode[mode](s, dim3(gx, l.co_blocks), prev.pool ? prev.pool : prev.act, w, d.bias, d.s, d.t, d.act, l.CI, l.CO,
                                                                 l.Hi, l.Wi, l.taps, l.pool == 2 ? 1 : 0, l.tl.TX, l.tl.tx_n, l.tl.tiles, h16 ? d.invh : 1.f,
                                                                 net.ovf(OVF_RANGE), net.d_ovfc, guard, items);
    if (l.pool == 3) {
        const size_t total = (size_t)m * l.H3 * l.W3 * (l.CO / 4);
        K_POOL3(s, std::min(cdiv(total, 256), 64 * n_cus), reinterpret_cast<const float4*>(d.act), reinterpret_cast<float4*>(d.pool), m, l.Ho, l.Wo, l.CO / 4, guard);
    }
}

}  // namespace

#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)      // a chain of allocations stops at its first failure
template <class T, class V>
static int up(Net* net, T** dst, const std::vector<V>& v, const char* who) {
    const int rc = net->weights.device_bytes(dst, v.size() * sizeof(V), who);
    if (rc != TREXHIP_OK) return rc;
    TH_CHECK_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice));
    return TREXHIP_OK;
}

// pack -> upload of a parsed blob into a new Net; *out stays null on a failure
static int arch_build(const ArchBlob& wb, const ArchPlan& plan, const char* who, Net** out) {
    *out = nullptr;
    Net* net = new Net();
    net->classes = wb.classes; net->W = wb.W; net->H = wb.H; net->CH = wb.CH;
    ArchNet* a = net->arch = new ArchNet();
    a->plan = plan;
    const ArchSpec& sp = *a->plan.spec;
    const bool fold = sp.bn2d && !sp.bn_behind_pool;
    int rc = TREXHIP_OK;
    for (int i = 0; i < sp.n_conv && rc == TREXHIP_OK; ++i) {
        const ArchLayerPlan& l = a->plan.L[i];
        ArchLayerDev& d = a->L[i];
        const int ci_real = i == 0 ? wb.CH : sp.conv[i - 1].CO;
        const ArchConvImage im = i == 0 ? pack_arch_conv1(wb.conv[i], sp.conv[i].CO, wb.CH, l.taps, l.CO, fold)
                                        : pack_arch_conv(wb.conv[i], sp.conv[i].CO, ci_real, l.taps, l.CO, l.CI, l.COB, fold);
        TRY(up(net, &d.w, im.w, who)); TRY(up(net, &d.bias, im.bias, who)); TRY(up(net, &d.s, im.s, who)); TRY(up(net, &d.t, im.t, who));
        if (i > 0) {
            TRY(up(net, &d.ws, pack_arch_bf16x3(im.w, l.COB), who));
            const ScaledImage h = pack_arch_f16x2(im.w, l.COB);
            d.invh = h.inv;
            TRY(up(net, &d.wh, h.v, who));
        }
    }
    const int P = sp.gap ? 1 : a->plan.Hf * a->plan.Wf;
    const Folded f1 = pack_arch_fc1(wb.fc1w, wb.fc1b, sp.hidden, a->plan.NH, sp.conv[sp.n_conv - 1].CO, a->plan.Cf, P);
    TRY(up(net, &a->wf1, f1.w, who)); TRY(up(net, &a->bf1, f1.b, who));
    const Folded bn = pack_arch_bn1d(wb.bn1d, sp.hidden, a->plan.NH);
    TRY(up(net, &a->hs, bn.w, who)); TRY(up(net, &a->ht, bn.b, who));
    TRY(up(net, &a->wf2t, pack_arch_fc2(wb.fc2w, wb.classes, sp.hidden), who));
    TRY(up(net, &a->bf2, std::vector<float>(wb.fc2b, wb.fc2b + wb.classes), who));
    TRY(net->weights.device_bytes(&net->d_ovf, ARCH_OVF_WORDS * 4, who));
    if (rc == TREXHIP_OK && hipMemset(net->d_ovf, 0, ARCH_OVF_WORDS * 4) != hipSuccess) rc = TREXHIP_E_DEVICE;
    if (rc != TREXHIP_OK) { free_net(net); return rc; }
    *out = net;
    return TREXHIP_OK;
}

int arch_load(trexhip_ctx* ctx, const void* blob, size_t bytes) {
    ArchBlob wb;
    const int prc = parse_arch_blob(blob, bytes, "trexhip_load_weights", &wb);
    if (prc != TREXHIP_OK) return prc;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    free_net(static_cast<Net*>(ctx->net));
    ctx->net = nullptr;
    Net* net;
    const int rc = arch_build(wb, arch_plan(wb.id, wb.W, wb.H, wb.CH), "trexhip_load_weights", &net);
    if (rc != TREXHIP_OK) return rc;
    ctx->net = net;
    return TREXHIP_OK;
}

// the category network: parsed and built BEFORE the loaded one is let go, so a refused blob leaves it in place; the identity slot is not touched
int category_load(trexhip_ctx* ctx, const void* blob, size_t bytes) {
    const char* who = "trexhip_categorize_load_weights";
    ArchBlob wb;
    const int prc = parse_category_blob(blob, bytes, who, &wb);
    if (prc != TREXHIP_OK) return prc;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    Net* net;
    const int rc = arch_build(wb, category_plan(wb.W, wb.H, wb.CH), who, &net);
    if (rc != TREXHIP_OK) return rc;
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));        // an earlier call may still run on the network that is replaced
    free_net(static_cast<Net*>(ctx->cat));
    ctx->cat = net;
    return TREXHIP_OK;
}

int arch_ensure_act(trexhip_ctx* ctx, Net* net, int n, const char* who) {
    if (n <= net->max_crops) return TREXHIP_OK;
    ArchNet& a = *net->arch;
    // (no captured chains to drop: these chains are not captured)
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));       // an earlier call may still read the buffers that are replaced here
    net->batch.free_all();
    net->h_probs = nullptr;
    net->max_crops = 0;
    Mem& B = net->batch;
    const size_t N = n, M = std::min(n, a.plan.chunk);
    int rc = B.device_bytes(&net->d_ovfc, M, who);
    for (int i = 0; i < a.plan.n_conv; ++i) {
        TRY(B.device_bytes(&a.L[i].act, M * a.plan.L[i].act_floats * 4, who));
        a.L[i].pool = nullptr;
        if (a.plan.L[i].pool == 3) TRY(B.device_bytes(&a.L[i].pool, M * a.plan.L[i].pool_floats * 4, who));
    }
    a.gap = nullptr;
    if (a.plan.spec->gap) TRY(B.device_bytes(&a.gap, M * a.plan.Cf * 4, who));
    TRY(B.device_bytes(&a.fc1, M * a.plan.NH * 4, who));
    TRY(B.device_bytes(&net->probs, N * net->classes * 4, who));
    TRY(B.device_bytes(&net->logits, N * net->classes * 4, who));
    TRY(B.device_bytes(&net->crops, N * net->W * net->H * net->CH, who));
    TRY(B.pinned(&net->h_probs, N * net->classes, who));
    a.labels = nullptr; a.h_labels = nullptr;
    if (a.plan.spec->id == ARCH_ID_CATEGORY) { TRY(B.device_bytes(&a.labels, N * 4, who)); TRY(B.pinned(&a.h_labels, N, who)); }
    if (rc != TREXHIP_OK) return rc;
    TH_CHECK_HIP(hipMemsetAsync(net->d_ovfc, 0, M, ctx->stream));
    net->max_crops = n;
    return TREXHIP_OK;
}
#undef TRY

int arch_forward(trexhip_ctx* ctx, const Net& net, const uint8_t* d_crops, int n, float* d_probs, float* d_logits, int32_t* d_labels) {
    const ArchNet& a = *net.arch;
    const bool cat = a.plan.spec->id == ARCH_ID_CATEGORY;      // normalised first layer, a label per crop, no share in the identity stages' times
    const ArchPlan& p = a.plan;
    if (!ctx->attr_cnn) {
        for (const LdsAttr& at : lds_attrs()) TH_CHECK_HIP(hipFuncSetAttribute(at.fn, hipFuncAttributeMaxDynamicSharedMemorySize, at.bytes));
        ctx->attr_cnn = true;
    }
    hipStream_t s = ctx->stream;
    const int mode = ctx->cnn_mode;
    const bool h16 = mode == TREXHIP_CNN_FP16X3;
    const size_t crop_bytes = (size_t)net.W * net.H * net.CH;
    if (!cat) stage_begin(ctx, TREXHIP_STAGE_CNN_ALL);
    if (h16) TH_CHECK_HIP(hipMemsetAsync(net.ovf(ARCH_STAT_RERUN), 0, 8, s));
    const ArchLayerPlan& l0 = p.L[0];
    const ArchLayerDev& last = a.L[p.n_conv - 1];
    for (int c0 = 0; c0 < n; c0 += p.chunk) {
        const int m = std::min(p.chunk, n - c0);
        (cat ? ARCH_CONV1_T3N : l0.taps == 3 ? ARCH_CONV1_T3 : ARCH_CONV1_T5)[net.CH](s, dim3(m * l0.tl.tiles, l0.co_blocks), d_crops + (size_t)c0 * crop_bytes, a.L[0].w, a.L[0].bias,
                                                              a.L[0].s, a.L[0].t, a.L[0].act, l0.CO, net.W, net.H, l0.pool == 2 ? 1 : 0, l0.tl.tx_n, l0.tl.tiles);
        for (int i = 1; i < p.n_conv; ++i) {       // (profiling: conv2 and conv3 have stages of their own, as in the V118_3 chains)
            const int stage = cat ? -1 : i == 1 ? TREXHIP_STAGE_CONV2 : i == 2 ? TREXHIP_STAGE_CONV3 : -1;
            if (stage >= 0) stage_begin(ctx, stage);
            launch_conv(s, net, a, i, mode, m, nullptr, ctx->n_cus);
            if (stage >= 0) stage_end(ctx, stage);
        }
        if (h16) {     // the guarded re-run of this chunk, in bf16x6 on the plan: every workgroup of it returns at once unless a crop left the fp16 range
            const uint32_t* g = net.ovf(OVF_PLAN);
            K_ARCH_GUARD_PLAN(s, 1, net.ovf(OVF_RANGE), net.d_ovfc, m, net.ovf(OVF_PLAN), net.ovf(ARCH_STAT_RERUN));
            for (int i = 1; i < p.n_conv; ++i) launch_conv(s, net, a, i, TREXHIP_CNN_BF16X6, m, g, ctx->n_cus);
        }
        const float* feat = last.pool ? last.pool : last.act;
        if (p.spec->gap) {
            K_GAP(s, cdiv((size_t)m * p.Cf, 256), feat, a.gap, m, p.Hf * p.Wf, p.Cf);
            feat = a.gap;
        }
        K_ARCH_FC1(s, dim3(cdiv(m, 32), p.NH / 32), feat, a.wf1, a.bf1, a.fc1, m, p.K, p.NH);
        K_ARCH_HEAD(s, cdiv(m, 4), a.fc1, a.hs, a.ht, a.wf2t, a.bf2, d_probs + (size_t)c0 * net.classes, d_logits ? d_logits + (size_t)c0 * net.classes : nullptr, m,
                    net.classes, p.NH, p.spec->hidden);
        if (d_labels) K_CAT_LABEL(s, cdiv(m, 4), d_logits + (size_t)c0 * net.classes, d_labels + c0, m, net.classes);       // (the caller hands logits with labels)
    }
    if (!cat) stage_end(ctx, TREXHIP_STAGE_CNN_ALL);
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

}  // namespace trexhip
