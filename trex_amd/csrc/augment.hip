// augment.hip -- the training loader of the identity network on the device (include/trexhip.h: trexhip_augment_device).
//
// Replaces TRexImageDataset.__getitem__ + DataLoader (Application/src/tracker/python/visual_recognition_torch.py:158-194, :1325-1337): a
// resident pool of uint8 crops and an index list -> the float32 NHWC batch of the training step, augmented like
//       transforms.RandomAffine(degrees=5, translate=(move_range, move_range))          nearest neighbour, fill 0, centre = image centre
//       transforms.ColorJitter(brightness, contrast, saturation = 0.85..1.15, hue = +-0.05)   on x = byte / 255, random order
// in torchvision's fp32 operation order (this file is compiled with -ffp-contract=off: every product and sum is rounded on its own, as
// torch's tensor operations round them).  ONE kernel, one workgroup per sample: draw (or read) the sample's parameters, stage the source
// crop in LDS, then one pass over the pixels per contrast operation (the operations in front of it, applied per pixel, feed the image
// mean it blends with) and a last pass that applies everything and writes.  The passes recompute the gather and the leading operations
// instead of keeping the image: the crop is in LDS, the arithmetic is a few dozen instructions, and nothing but the source bytes is read
// and nothing but the result written (1 + 4 bytes per pixel-channel).  The source coordinates are computed in fp64 (two products per
// axis and pixel), so the nearest-neighbour choice is the exact formula's except within ~1e-13 px of a tie.
#include "internal.h"
#include <cmath>
#include <string>

namespace trexhip {

enum { AUG_THREADS = 256, AUG_STAGE_MAX = 48 * 1024 };      // crops up to 48 KiB (128 x 128 x 3) are staged in LDS; larger ones gather from global memory

struct AugCfg {
    int W, H, HW, HWC;
    int augment;            // 0 = validation loader: d_out = float(byte)
    int draws_given;
    int staged, vec_in16;   // source crop goes through LDS; with 16-byte loads
    int vec_out;            // H*W a multiple of 4 and d_out 16-byte aligned: float4 stores
    int vec_plain;          // validation loader: 4 bytes in, float4 out
    trexhip_augment_params ap;
    uint64_t counter;
};

// the splitmix64 finaliser of k_t_masks (train.hip) over (seed, counter, sample, field) -> U[0, 1) with 24 bits
__device__ __forceinline__ float aug_uniform(uint64_t seed, uint64_t counter, uint32_t sample, uint32_t field) {
    uint64_t zed = seed + 0x9E3779B97F4A7C15ull * (counter * 0x100000001B3ull + ((uint64_t)sample * 8 + field) + 1);
    zed = (zed ^ (zed >> 30)) * 0xBF58476D1CE4E5B9ull;
    zed = (zed ^ (zed >> 27)) * 0x94D049BB133111EBull;
    zed ^= zed >> 31;
    return (float)(zed >> 40) * (1.0f / 16777216.0f);
}

__device__ __forceinline__ float aug_range(float lo, float hi, float u) { return lo + (hi - lo) * u; }     // torch's uniform_(lo, hi)

// RandomAffine.get_params + ColorJitter.get_params for one sample
__device__ trexhip_augment_draw aug_draw(const AugCfg& c, uint32_t sample) {
    const trexhip_augment_params& a = c.ap;
    trexhip_augment_draw d;
    d.angle = aug_range(-a.degrees, a.degrees, aug_uniform(a.seed, c.counter, sample, 0));
    const float mx = a.translate_x * (float)c.W, my = a.translate_y * (float)c.H;
    d.tx = (int32_t)rintf(aug_range(-mx, mx, aug_uniform(a.seed, c.counter, sample, 1)));              // int(round(.)): half to even
    d.ty = (int32_t)rintf(aug_range(-my, my, aug_uniform(a.seed, c.counter, sample, 2)));
    d.brightness = aug_range(a.brightness_lo, a.brightness_hi, aug_uniform(a.seed, c.counter, sample, 3));
    d.contrast = aug_range(a.contrast_lo, a.contrast_hi, aug_uniform(a.seed, c.counter, sample, 4));
    d.saturation = aug_range(a.saturation_lo, a.saturation_hi, aug_uniform(a.seed, c.counter, sample, 5));
    d.hue = aug_range(a.hue_lo, a.hue_hi, aug_uniform(a.seed, c.counter, sample, 6));
    // torch.randperm(4): the k-th of the 24 permutations, k uniform, by its Lehmer code
    int k = (int)(aug_uniform(a.seed, c.counter, sample, 7) * 24.0f);
    k = k > 23 ? 23 : k;
    int left = 0xE4;                                     // the unused operations 0, 1, 2, 3, two bits each
    int order = 0;
    for (int j = 0, radix = 6, rest = 4; j < 4; ++j) {
        const int pick = k / radix;
        k -= pick * radix;
        order |= ((left >> (2 * pick)) & 3) << (2 * j);
        left = (left & ((1 << (2 * pick)) - 1)) | ((left >> (2 * pick + 2)) << (2 * pick));           // take it out
        --rest;
        radix = rest > 1 ? radix / rest : 1;
    }
    d.order = order;
    return d;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float gray_of(const float* x) { return 0.2989f * x[0] + 0.587f * x[1] + 0.114f * x[2]; }      // rgb_to_grayscale

// torchvision's adjust_hue on one pixel: _rgb2hsv, h = (h + f) % 1, _hsv2rgb
__device__ __forceinline__ void hue_shift(float* x, float f) {
    const float r = x[0], g = x[1], b = x[2];
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.0f : maxc);
    const float div = eq ? 1.0f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    const float hr = maxc == r ? bc - gc : 0.0f;
    const float hg = (maxc == g && maxc != r) ? 2.0f + rc - bc : 0.0f;
    const float hb = (maxc != g && maxc != r) ? 4.0f + gc - rc : 0.0f;
    float h = hr + hg + hb;
    h = fmodf(h / 6.0f + 1.0f, 1.0f);
    h = fmodf(h + f, 1.0f);                               // torch's %: the sign of the divisor
    if (h < 0.0f) h += 1.0f;
    const float v = maxc;
    const float h6 = h * 6.0f;
    const float fl = floorf(h6);
    const float ff = h6 - fl;
    const int i = ((int)fl) % 6;
    const float p = clamp01(v * (1.0f - s));
    const float q = clamp01(v * (1.0f - s * ff));
    const float t = clamp01(v * (1.0f - (s * (1.0f - ff))));
    x[0] = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
    x[1] = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    x[2] = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// operations [0, upto) of the draw's order on one pixel; mean[k] = the image mean a contrast at position k blends with
template <int C>
__device__ __forceinline__ void jitter(float* x, const trexhip_augment_draw& d, int upto, const float* mean) {
    for (int k = 0; k < upto; ++k) {
        const int op = (d.order >> (2 * k)) & 3;
        if (op == 0) {
            for (int c = 0; c < C; ++c) x[c] = clamp01(d.brightness * x[c]);
        } else if (op == 1) {
            const float other = (1.0f - d.contrast) * mean[k];
            for (int c = 0; c < C; ++c) x[c] = clamp01(d.contrast * x[c] + other);
        } else if (C == 3 && op == 2) {
            const float other = (1.0f - d.saturation) * gray_of(x);
            for (int c = 0; c < C; ++c) x[c] = clamp01(d.saturation * x[c] + other);
        } else if (C == 3) {
            hue_shift(x, d.hue);
        }
    }
}

struct AugGeom { double c, s, ox, oy; };       // source = (c xo + s yo + ox, -s xo + c yo + oy), xo / yo relative to the image centre

// F.affine's inverse map + grid_sample(nearest, zeros, align_corners=False) for output pixel p -> x[C] = byte / 255, 0 outside
template <int C>
__device__ __forceinline__ void gather(const AugCfg& cfg, const AugGeom& g, const uint8_t* __restrict__ src, const uint8_t* lds, int p, float* x) {
    const int j = p / cfg.W, i = p - j * cfg.W;
    const double xo = (double)i - 0.5 * cfg.W + 0.5, yo = (double)j - 0.5 * cfg.H + 0.5;
    const double fx = rint(g.c * xo + g.s * yo + g.ox), fy = rint(-g.s * xo + g.c * yo + g.oy);
    if (fx >= 0.0 && fx <= (double)(cfg.W - 1) && fy >= 0.0 && fy <= (double)(cfg.H - 1)) {              // (false for NaN)
        const int o = ((int)fy * cfg.W + (int)fx) * C;
        for (int c = 0; c < C; ++c) x[c] = (float)(cfg.staged ? lds[o + c] : src[o + c]) / 255.0f;
    } else {
        for (int c = 0; c < C; ++c) x[c] = 0.0f;
    }
}

template <int C>
__global__ __launch_bounds__(AUG_THREADS) void k_augment(AugCfg cfg, const uint8_t* __restrict__ pool, const int32_t* __restrict__ pool_targets,
                                                         const int32_t* __restrict__ idx, trexhip_augment_draw* __restrict__ draws,
                                                         float* __restrict__ out, int32_t* __restrict__ targets_out) {
    extern __shared__ uint4 s_dyn[];
    __shared__ double s_part[AUG_THREADS / 64];
    const int tid = threadIdx.x;
    const uint32_t sample = blockIdx.x;
    const int entry = idx ? idx[sample] : (int)sample;                                   // range-checked on the host
    const uint8_t* __restrict__ src = pool + (size_t)entry * cfg.HWC;
    float* __restrict__ dst = out + (size_t)sample * cfg.HWC;
    if (tid == 0 && targets_out) targets_out[sample] = pool_targets[entry];

    if (!cfg.augment) {                                                                 // transform=None: x.div(255).clamp(0, 1) * 255 == float(byte)
        if (cfg.vec_plain) {
            for (int e = tid; e < cfg.HWC / 4; e += AUG_THREADS) {
                const uchar4 b = reinterpret_cast<const uchar4*>(src)[e];
                reinterpret_cast<float4*>(dst)[e] = make_float4((float)b.x, (float)b.y, (float)b.z, (float)b.w);
            }
        } else {
            for (int e = tid; e < cfg.HWC; e += AUG_THREADS) dst[e] = (float)src[e];
        }
        return;
    }

    trexhip_augment_draw d;
    if (cfg.draws_given) d = draws[sample];
    else {
        d = aug_draw(cfg, sample);
        if (tid == 0 && draws) draws[sample] = d;
    }
    AugGeom g;
    {
        const double rad = (double)d.angle * (3.14159265358979323846 / 180.0);
        g.c = cos(rad);
        g.s = sin(rad);
        g.ox = -g.c * d.tx - g.s * d.ty + 0.5 * cfg.W - 0.5;
        g.oy = g.s * d.tx - g.c * d.ty + 0.5 * cfg.H - 0.5;
    }
    const uint8_t* lds = reinterpret_cast<const uint8_t*>(s_dyn);
    if (cfg.staged) {
        if (cfg.vec_in16) for (int e = tid; e < cfg.HWC / 16; e += AUG_THREADS) s_dyn[e] = reinterpret_cast<const uint4*>(src)[e];
        else for (int e = tid; e < cfg.HWC; e += AUG_THREADS) reinterpret_cast<uint8_t*>(s_dyn)[e] = src[e];
        __syncthreads();
    }

    // one reduction pass per contrast operation (a permutation has exactly one): the image mean "as it stands at that point", summed in
    // a fixed order -- per thread its pixels in index order, per wave a butterfly, the four waves in order -- so a repeat gives the same bits
    float mean[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int groups = (cfg.HW + 3) / 4;
    for (int k = 0; k < 4; ++k) {
        if (((d.order >> (2 * k)) & 3) != 1) continue;
        double part = 0.0;
        for (int grp = tid; grp < groups; grp += AUG_THREADS)
            for (int p = 4 * grp; p < min(4 * grp + 4, cfg.HW); ++p) {
                float x[C];
                gather<C>(cfg, g, src, lds, p, x);
                jitter<C>(x, d, k, mean);
                part += (double)(C == 3 ? gray_of(x) : x[0]);
            }
        for (int m = 1; m < 64; m <<= 1) part += __shfl_xor(part, m);
        __syncthreads();                                    // (the previous pass's readers of s_part are done)
        if ((tid & 63) == 0) s_part[tid >> 6] = part;
        __syncthreads();
        double total = 0.0;
        for (int w = 0; w < AUG_THREADS / 64; ++w) total += s_part[w];
        mean[k] = (float)(total / (double)cfg.HW);
    }

    // everything applied, clamp(0, 1) * 255, four pixels (4 C floats, contiguous) per thread and step
    for (int grp = tid; grp < groups; grp += AUG_THREADS) {
        float v[4 * C];
        const int p0 = 4 * grp, np = min(4, cfg.HW - p0);
        for (int q = 0; q < 4; ++q) {
            if (q >= np) break;
            float x[C];
            gather<C>(cfg, g, src, lds, p0 + q, x);
            jitter<C>(x, d, 4, mean);
            for (int c = 0; c < C; ++c) v[q * C + c] = clamp01(x[c]) * 255.0f;
        }
        if (cfg.vec_out && np == 4) {
            float4* o4 = reinterpret_cast<float4*>(dst + (size_t)p0 * C);
            for (int e = 0; e < C; ++e) o4[e] = make_float4(v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]);
        } else {
            for (int e = 0; e < np * C; ++e) dst[(size_t)p0 * C + e] = v[e];
        }
    }
}

static bool range_ok(float lo, float hi, float min_lo, float max_hi) { return std::isfinite(lo) && std::isfinite(hi) && lo <= hi && lo >= min_lo && hi <= max_hi; }

}  // namespace trexhip

using namespace trexhip;

extern "C" {

void trexhip_default_augment_params(trexhip_augment_params* p, int32_t width, int32_t height) {
    if (!p) return;
    const int m = width < height ? width : height;
    const float move_range = m > 0 ? (float)std::fmin(0.05, 2.0 / m) : 0.05f;           // visual_recognition_torch.py:1301
    *p = trexhip_augment_params{5.0f, move_range, move_range, 0.85f, 1.15f, 0.85f, 1.15f, 0.85f, 1.15f, -0.05f, 0.05f, 0};
}

int trexhip_augment_device(trexhip_ctx* ctx, const trexhip_augment_params* ap, const uint8_t* d_pool, const int32_t* d_pool_targets,
                           int32_t pool_size, const int32_t* indices, int32_t n, int32_t width, int32_t height, int32_t channels,
                           trexhip_augment_draw* d_draws, int32_t draws_given, uint64_t counter, float* d_out, int32_t* d_targets_out) {
    if (!ctx || !d_pool || !d_out) { set_error("trexhip_augment_device: null argument"); return TREXHIP_E_INVALID; }
    if (width < 8 || width > 256 || height < 8 || height > 256) { set_error("trexhip_augment_device: image sizes from 8 x 8 to 256 x 256 only"); return TREXHIP_E_UNSUPPORTED; }
    if (channels != 1 && channels != 3) { set_error("trexhip_augment_device: 1 or 3 channels only"); return TREXHIP_E_UNSUPPORTED; }
    if (n < 1 || pool_size < 1) { set_error("trexhip_augment_device: need n >= 1 samples from a pool of at least one crop"); return TREXHIP_E_INVALID; }
    if ((d_pool_targets == nullptr) != (d_targets_out == nullptr)) { set_error("trexhip_augment_device: pool targets and batch targets come together"); return TREXHIP_E_INVALID; }
    if (ap) {
        if (!(std::isfinite(ap->degrees) && ap->degrees >= 0.0f) || !range_ok(0.0f, ap->translate_x, 0.0f, 1.0f) || !range_ok(0.0f, ap->translate_y, 0.0f, 1.0f)) {
            set_error("trexhip_augment_device: degrees must be >= 0 and translate within 0..1"); return TREXHIP_E_INVALID;
        }
        if (!range_ok(ap->brightness_lo, ap->brightness_hi, 0.0f, INFINITY) || !range_ok(ap->contrast_lo, ap->contrast_hi, 0.0f, INFINITY) ||
            !range_ok(ap->saturation_lo, ap->saturation_hi, 0.0f, INFINITY) || !range_ok(ap->hue_lo, ap->hue_hi, -0.5f, 0.5f)) {
            set_error("trexhip_augment_device: brightness / contrast / saturation need 0 <= lo <= hi, hue -0.5 <= lo <= hi <= 0.5"); return TREXHIP_E_INVALID;
        }
        if (draws_given && !d_draws) { set_error("trexhip_augment_device: draws_given without d_draws"); return TREXHIP_E_INVALID; }
    }
    if (indices) {
        for (int i = 0; i < n; ++i)
            if (indices[i] < 0 || indices[i] >= pool_size) {
                set_error("trexhip_augment_device: indices[" + std::to_string(i) + "] = " + std::to_string(indices[i]) + " is outside the pool of " + std::to_string(pool_size));
                return TREXHIP_E_INVALID;
            }
    } else if (n > pool_size) {
        set_error("trexhip_augment_device: without indices the batch is pool entries 0 .. n-1: n exceeds pool_size"); return TREXHIP_E_INVALID;
    }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    const int32_t* d_idx = nullptr;
    if (indices) {
        if (int rc = ctx->aug_idx.reserve(ctx, (size_t)std::max(n, 1024) * sizeof(int32_t), "trexhip_augment_device")) return rc;   // at least 1024 entries: typical batches never grow it
        TH_CHECK_HIP(hipMemcpyAsync(ctx->aug_idx.p, indices, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));   // pageable source: staged before the call returns
        d_idx = ctx->aug_idx.as<int32_t>();
    }
    AugCfg c{};
    c.W = width; c.H = height; c.HW = width * height; c.HWC = c.HW * channels;
    c.augment = ap ? 1 : 0;
    c.draws_given = draws_given ? 1 : 0;
    c.staged = (ap && c.HWC <= AUG_STAGE_MAX) ? 1 : 0;
    const uintptr_t pin = reinterpret_cast<uintptr_t>(d_pool), pout = reinterpret_cast<uintptr_t>(d_out);
    c.vec_in16 = (c.HWC % 16 == 0 && pin % 16 == 0) ? 1 : 0;
    c.vec_out = (c.HW % 4 == 0 && pout % 16 == 0) ? 1 : 0;
    c.vec_plain = (c.HWC % 4 == 0 && pin % 4 == 0 && pout % 16 == 0) ? 1 : 0;
    if (ap) c.ap = *ap;
    c.counter = counter;
    const size_t lds = c.staged ? (size_t)((c.HWC + 15) / 16) * 16 : 0;
    if (channels == 3) hipLaunchKernelGGL(k_augment<3>, dim3(n), dim3(AUG_THREADS), lds, ctx->stream, c, d_pool, d_pool_targets, d_idx, ap ? d_draws : nullptr, d_out, d_targets_out);
    else               hipLaunchKernelGGL(k_augment<1>, dim3(n), dim3(AUG_THREADS), lds, ctx->stream, c, d_pool, d_pool_targets, d_idx, ap ? d_draws : nullptr, d_out, d_targets_out);
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

}  // extern "C"
