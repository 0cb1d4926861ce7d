// train_any.hip -- the kernels of the identity network V118_3's training step that follow the individual_image_size: W, H = 8..256 at run
// time, square or not, CH = 1 or 3, NHWC fp32 throughout, exact fp32 arithmetic.  Every pool floors like nn.MaxPool2d(2).
// The BN / pool and fc1 kernels run at every size, 80x80 included; the convolutions and weight gradients at every size but 80x80, where
// train.hip keeps its own (other tilings, another summation order, the fp16 two-piece path), as cnn.hip does beside cnn_any.hip.
//
// The tap count of every convolution kernel is a template parameter: 5 (V118_3, v100, v110) or 3 (the category network, train_arch.hip), whose conv1
// pair also normalises its input and whose block kernels read element-wise dropout masks.
//
//   k_tany_conv1       CH -> 16 on the VALU, raw output + bias: one workgroup per (crop, 16 x 16 pixels), patch in LDS
//   k_tany_conv<>      conv2 / conv3 forward and both data gradients: TAPS^2 shifted GEMMs on v_mfma_f32_32x32x2_f32, the 2-D tiles of
//                      k_any_conv (cnn_any.hip) with a raw epilogue
//   k_tany_wgrad<>     conv2 / conv3 weight gradients on the same instruction, operands straight from L2, partials per share of the batch
//   k_tany_wgrad1      conv1 weight gradient: k_t_wgrad1's sliding window on bands of 8 rows x strips of 64 columns
//   k_tany_bn_pool, k_tany_pool_bwd_stats, k_tany_bn_bwd    BN + ReLU + pool + dropout and its way back on planes of h x w pixels (every size)
//   k_tany_fc1, _wgrad, _dgrad                              fc1 at P = (H/8)(W/8) positions (every size)
//   k_tany_fc1_sum                                          its partial planes added up (not at 80x80: the head adds the 100 itself)
// k_t_bn_stats, k_t_red_finalize, k_t_wgrad_reduce, k_t_reduce, k_t_repack_bwd, the head, the masks and Adam are train.hip's own: they do
// not depend on the size.
//
// Three things such a chain gets wrong, and where each is handled:
//   1. Pixels outside every pool window.  With an odd h or w the last row / column of z lies in no 2x2 window: the pool hands it no
//      gradient, but its dz is not zero -- BN's backward subtracts the batch means from every pixel (k_tany_bn_bwd walks ceil(h/2) x
//      ceil(w/2) windows and masks), and those pixels enter the batch statistics (k_t_bn_stats runs over all n h w rows), the weight
//      gradient (k_tany_wgrad / k_tany_wgrad1 walk every pixel) and the data gradient (k_tany_conv's tiles cover ceil, not floor).
//   2. Successive floors.  W -> W/2 -> (W/2)/2 -> ((W/2)/2)/2, so 21 gives 10, 5, 2: every level has its own odd edge.  No kernel derives a
//      level's size from another level's: each gets the (h, w) of its plane from TrainAnyGeom (train_geom.h).
//   3. Determinism.  Every sum has a fixed order that depends on the size (and, for the sums over the batch, on n) alone: column sums per
//      workgroup + k_t_red_finalize, weight-gradient partials per contiguous share of the batch's rows + k_t_wgrad_reduce / k_t_reduce, fc1's
//      partial planes added in position order by k_tany_fc1_sum.  No floating-point atomics, no tickets.
#include "internal.h"
#include "conv_f32.h"
#include "train_dev.h"
#include "train_any.h"

namespace trexhip {
namespace {

// ------------------------------------------------------------------------------------------------
// conv1 forward: [n][H][W][CH] -> z1 [n][H][W][16] = conv + bias (k_any_conv1's patch-in-LDS walk without the fold and the pool)
// ------------------------------------------------------------------------------------------------
// the first layer's input as both conv1 kernels stage it.  NORM (the category network, trex_learn_category.py:289 "images / 127.5 - 1"): a pixel
// inside the crop is a true fp32 division and a subtraction, k_arch_conv1<.., NORM = true>'s expression (cnn_arch.hip), and the zero padding is
// applied to the NORMALISED image, so a pixel outside the crop is 0 and not -1
template <bool NORM>
__device__ __forceinline__ float tany_input(const float v) { return NORM ? __fsub_rn(__fdiv_rn(v, 127.5f), 1.0f) : v; }

template <int CH, int TAPS = 5, bool NORM = false>
__global__ __launch_bounds__(256) void k_tany_conv1(const float* __restrict__ x, const float* __restrict__ w /*[CH][TAPS^2][16]*/, const float* __restrict__ b,
                                                    float* __restrict__ z, const int W, const int H, const int tx_n, const int tiles) {
    constexpr int PW = TA_C1T + TAPS - 1, T2 = TAPS * TAPS;
    __shared__ __attribute__((aligned(16))) float wl[CH * T2 * 16];
    __shared__ float img[CH * PW * PW];
    const int crop = blockIdx.x / tiles, t = blockIdx.x - crop * tiles;
    const int ty = t / tx_n, tx = t - ty * tx_n;
    const int y0 = TA_C1T * ty - TAPS / 2, x0 = TA_C1T * tx - TAPS / 2;
    const float* src = x + (size_t)crop * H * W * CH;
    for (int i = threadIdx.x; i < CH * T2 * 16; i += 256) wl[i] = w[i];
    for (int i = threadIdx.x; i < PW * PW * CH; i += 256) {
        const int c = i % CH, p = i / CH, py = p / PW, px = p - py * PW;
        const int iy = y0 + py, ix = x0 + px;
        img[c * PW * PW + p] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? tany_input<NORM>(src[((size_t)iy * W + ix) * CH + c]) : 0.f;      // zero padding ('same')
    }
    __syncthreads();
    const int py = threadIdx.x / TA_C1T, px = threadIdx.x % TA_C1T;
    const int oy = TA_C1T * ty + py, ox = TA_C1T * tx + px;
    if (oy >= H || ox >= W) return;                                   // ragged last tiles
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
#pragma unroll 1
    for (int c = 0; c < CH; ++c)
#pragma unroll 1
        for (int ky = 0; ky < TAPS; ++ky)
#pragma unroll
            for (int kx = 0; kx < TAPS; ++kx) {
                const float v = img[c * PW * PW + (py + ky) * PW + px + kx];
                const float4* wv = reinterpret_cast<const float4*>(wl + (c * T2 + ky * TAPS + kx) * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 t4 = wv[q];
                    acc[4 * q] += v * t4.x; acc[4 * q + 1] += v * t4.y; acc[4 * q + 2] += v * t4.z; acc[4 * q + 3] += v * t4.w;
                }
            }
    float4* o = reinterpret_cast<float4*>(z + (((size_t)crop * H + oy) * W + ox) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = make_float4(acc[4 * q] + b[4 * q], acc[4 * q + 1] + b[4 * q + 1], acc[4 * q + 2] + b[4 * q + 2], acc[4 * q + 3] + b[4 * q + 3]);
}

// ------------------------------------------------------------------------------------------------
// conv2 / conv3 forward and data gradients: in [n][Hi][Wi][CI] -> out [n][Hi][Wi][COUT] = TAPS x TAPS 'same' convolution (+ bias), exact fp32 on
// the matrix cores.  k_any_conv<.., KIND 2, ..>'s walk: a tile is 64 pool windows = 256 pixels (8 M-tiles of 32, window-major) shaped
// 4 x 16, 8 x 8 or 16 x 4 windows, its patch (at most 36 x 12 pixels x CIC channels at 5 taps) in LDS, the weights of one tap double-buffered.
// The tiles cover ceil(Hi / 2) x ceil(Wi / 2) windows: the odd last row / column belongs to no pool window but is an output like any
// other (a raw epilogue stores all four pixels of a window, masked by y < Hi and x < Wi).  COUT < CO: the data gradient of conv2 has 16
// real channels in a 32-wide tile
// ------------------------------------------------------------------------------------------------
constexpr int TA_APMAX = 36 * 12;

template <int CO, int CIC>
struct TanyGeom {
    static constexpr int PSTRIDE = CIC + 1;                           // floats per patch pixel: odd, conflict-free b32 reads
    static constexpr int PATCH = TA_APMAX * PSTRIDE;                  // floats
    static constexpr int BT = CIC * CO;                               // floats per weight tile (one tap of one chunk)
    static constexpr int BV = BT / 4;
    static constexpr int BPT = (BV + 511) / 512;
    static constexpr int NT = CO / 32, WM = 8 / NT, TPW = 8 / WM;     // 8 waves: NT along N, WM along M, TPW M-tiles each
    static constexpr int LDS_BYTES = (PATCH + 2 * BT) * 4;
};

template <int CI, int CO, int CIC, int COUT, int TAPS = 5>
__global__ __launch_bounds__(512) void k_tany_conv(const float* __restrict__ in, const float* __restrict__ wp /*[CI/CIC][TAPS^2][CIC][CO]*/,
                                                   const float* __restrict__ bias /*[COUT] or null*/, float* __restrict__ out, const int Hi, const int Wi,
                                                   const int TX, const int tx_n, const int tiles) {
    using G = TanyGeom<CO, CIC>;
    constexpr int Q4 = CIC / 4, T2 = TAPS * TAPS, HALO = TAPS / 2;
    static_assert(T2 % 2 == 1, "the last tap of a chunk sits in buffer 0, where the next chunk's first tap is staged behind the barrier");
    extern __shared__ __attribute__((aligned(16))) float tany_lds[];
    float* patch = tany_lds;
    float* Bs = tany_lds + G::PATCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = wave % G::NT, mg = wave / G::NT;
    const int TY = AW / TX, PW = 2 * TX + TAPS - 1, PH = 2 * TY + TAPS - 1;      // PH * PW <= TA_APMAX for TX = 4, 8, 16 at 5 taps, less at 3
    int aoff[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int p = (mg + G::WM * m) * 32 + j;                        // window-major pixel index of the tile, < 256
        const int wi = p >> 2, sub = p & 3;
        const int wy = wi / TX, wx = wi - wy * TX;
        aoff[m] = ((2 * wy + (sub >> 1)) * PW + (2 * wx + (sub & 1))) * G::PSTRIDE + h;
    }
    const int crop = blockIdx.x / tiles, t = blockIdx.x - crop * tiles;
    const int ty = t / tx_n, tx = t - ty * tx_n;
    const int py0 = 2 * ty * TY, px0 = 2 * tx * TX;                     // first pixel of the tile
    const int iy0 = py0 - HALO, ix0 = px0 - HALO;                       // first input pixel of its patch
    f32x16 acc[G::TPW];
#pragma unroll
    for (int m = 0; m < G::TPW; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    const float* inc = in + (size_t)crop * Hi * Wi * CI;
    for (int cc = 0; cc < CI / CIC; ++cc) {
        __syncthreads();
        for (int idx = tid; idx < PH * PW * Q4; idx += 512) {
            const int q = idx % Q4, px = idx / Q4;
            const int py = px / PW, pxx = px - py * PW;
            const int iy = iy0 + py, ix = ix0 + pxx;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                 // zero padding ('same'), and the rows / columns past a ragged edge
            if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) v = *reinterpret_cast<const float4*>(inc + ((size_t)iy * Wi + ix) * CI + cc * CIC + q * 4);
            float* d = patch + px * G::PSTRIDE + q * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        const float4* wsrc = reinterpret_cast<const float4*>(wp) + (size_t)cc * T2 * G::BV;
        for (int i = tid; i < G::BV; i += 512) reinterpret_cast<float4*>(Bs)[i] = wsrc[i];
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < T2; ++tap) {
            const int buf = tap & 1;
            float4 nb[G::BPT];
            if (tap < T2 - 1) {
#pragma unroll
                for (int u = 0; u < G::BPT; ++u) { const int i = tid + u * 512; if (i < G::BV) nb[u] = wsrc[(size_t)(tap + 1) * G::BV + i]; }
            }
            const float* asrc = patch + ((tap / TAPS) * PW + (tap % TAPS)) * G::PSTRIDE;
            const float* bsrc = Bs + buf * G::BT + h * CO + n * 32 + j;
#pragma unroll
            for (int t2 = 0; t2 < CIC / 2; ++t2) {                      // input channel 2 t2 + h of the chunk
                const float bq = bsrc[2 * t2 * CO];
#pragma unroll
                for (int m = 0; m < G::TPW; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(asrc[aoff[m] + 2 * t2], bq, acc[m], 0, 0, 0);
            }
            if (tap < T2 - 1) {
#pragma unroll
                for (int u = 0; u < G::BPT; ++u) { const int i = tid + u * 512; if (i < G::BV) reinterpret_cast<float4*>(Bs + (buf ^ 1) * G::BT)[i] = nb[u]; }
            }
            __syncthreads();
        }
    }
    // raw epilogue: lane (j, h) holds in registers 4 g + sub the four pixels of window mt * 8 + 2 g + h, channel n * 32 + j
    const int co = n * 32 + j;
    if (co >= COUT) return;
    const float bz = bias ? bias[co] : 0.f;
    float* oc = out + (size_t)crop * Hi * Wi * COUT;
#pragma unroll
    for (int m = 0; m < G::TPW; ++m) {
        const int mt = mg + G::WM * m;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int wi = mt * 8 + 2 * g + h;
            const int wy = wi / TX, wx = wi - wy * TX;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) {
                const int y = py0 + 2 * wy + (sub >> 1), xx = px0 + 2 * wx + (sub & 1);
                if (y < Hi && xx < Wi) oc[((size_t)y * Wi + xx) * COUT + co] = acc[m][4 * g + sub] + bz;      // the odd last row / column included
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// conv2 / conv3 weight gradient: g[tap][ci][co] = sum over n, y, x of a[n][y + ky - TAPS/2][x + kx - TAPS/2][ci] * dz[n][y][x][co], zero padding, fp32
// MFMA with the pixels as the contraction (one 32x32x2 step = two neighbouring pixels of a row), operands straight from L2.
// Workgroup type (blockIdx.x) = kernel row ky x 32-wide slice of the input channels; wave = TT taps of that row (CI 16: two taps x 16
// channels fill the 32 rows of a tile, kx = TAPS is masked); a wave holds all CO / 32 output tiles.  Share (blockIdx.y) = `per` consecutive rows
// of the batch (row = crop * Hi + y), walked in order: part[share][tap][ci][co].  Every pixel of dz is walked, the ones outside every pool
// window too
// ------------------------------------------------------------------------------------------------
template <int CI, int TAPS = 5>
struct TanyWgradGeom {
    static constexpr int CIS = CI < 32 ? CI : 32, TT = 32 / CIS, NW = (TAPS + TT - 1) / TT, CT = CI / CIS;
};

template <int CI, int CO, int TAPS = 5>
__global__ __launch_bounds__(320) void k_tany_wgrad(const float* __restrict__ a /*[n][Hi][Wi][CI]*/, const float* __restrict__ dz /*[n][Hi][Wi][CO]*/,
                                                    float* __restrict__ part, const int rows /*n * Hi*/, const int per, const int Hi, const int Wi) {
    using G = TanyWgradGeom<CI, TAPS>;
    constexpr int NT = CO / 32, T2 = TAPS * TAPS, HALO = TAPS / 2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, j = lane & 31, h = lane >> 5;
    const int ky = blockIdx.x / G::CT, ct = blockIdx.x % G::CT;
    const int kx = wv * G::TT + j / G::CIS, ci = ct * G::CIS + j % G::CIS;
    const bool kx_ok = kx < TAPS;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
    for (int r = r0; r < r1; ++r) {
        const int crop = r / Hi, y = r - crop * Hi;
        const int ay = y + ky - HALO;
        if (ay < 0 || ay >= Hi) continue;                               // (uniform) the kernel row looks at the zero padding
        const float* arow = a + ((size_t)crop * Hi + ay) * Wi * CI + ci;
        const float* drow = dz + (size_t)r * Wi * CO + j;
#pragma unroll 4
        for (int x0 = 0; x0 < Wi; x0 += 2) {
            const int x = x0 + h, ax = x + kx - HALO;
            const bool xok = x < Wi;                                    // an odd Wi: the pair's second pixel is past the row
            const float av = (kx_ok && xok && ax >= 0 && ax < Wi) ? arow[(size_t)ax * CI] : 0.f;
            float bv[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = xok ? drow[(size_t)x * CO + nt * 32] : 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[nt], acc[nt], 0, 0, 0);
        }
    }
    float* pp = part + (size_t)blockIdx.y * T2 * CI * CO;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = 8 * (r / 4) + 4 * h + (r % 4);                 // accumulator r of lane (j, h) is row 8 (r / 4) + 4 h + r % 4
            const int kxm = wv * G::TT + m / G::CIS, cim = ct * G::CIS + m % G::CIS;
            if (kxm < TAPS) pp[((size_t)(ky * TAPS + kxm) * CI + cim) * CO + nt * 32 + j] = acc[nt][r];
        }
}

// ------------------------------------------------------------------------------------------------
// conv1 weight gradient (VALU): k_t_wgrad1's sliding window at run-time W and H.  Block = 8 rows x 64 columns of one crop ->
// part[block][c][tap][16]; rows and columns past the image hold dz = 0, the window's halo outside the image x = 0
// ------------------------------------------------------------------------------------------------
template <int CH, int TAPS = 5, bool NORM = false>
__global__ __launch_bounds__(512) void k_tany_wgrad1(const float* __restrict__ x /*[n][H][W][CH]*/, const float* __restrict__ dz /*[n][H][W][16]*/,
                                                     float* __restrict__ part, const int W, const int H, const int tx_n, const int tiles) {
    // NORM: dz multiplies the image conv1 saw -- normalised inside the crop, 0 outside it (tany_input)
    constexpr int R = TA_WG1_ROWS, CW = TA_WG1_COLS, HALO = TAPS / 2, PW = CW + 2 * HALO, T2 = TAPS * TAPS;
    constexpr int TW = T2 * 16;                                        // words of one channel's gradient: 400 at 5 taps, 144 at 3
    constexpr int ACT = 4 * TAPS * 16;                                 // working threads: 4 row pairs x kernel row x output channel
    static_assert(4 * CH * TW <= R * CW * 16, "the row pairs' exchange fits in ds");
    __shared__ float xs[(R + 2 * HALO) * PW * CH];
    __shared__ __attribute__((aligned(16))) float ds[R * CW * 16];
    const int tid = threadIdx.x, crop = blockIdx.x / tiles, t = blockIdx.x - crop * tiles;
    const int row0 = (t / tx_n) * R, col0 = (t % tx_n) * CW;
    for (int idx = tid; idx < (R + 2 * HALO) * PW * CH; idx += 512) {
        const int c = idx % CH, px = (idx / CH) % PW, py = idx / (CH * PW);
        const int iy = row0 + py - HALO, ix = col0 + px - HALO;
        xs[idx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? tany_input<NORM>(x[(((size_t)crop * H + iy) * W + ix) * CH + c]) : 0.f;
    }
    for (int idx = tid; idx < R * CW * 4; idx += 512) {
        const int q = idx & 3, xx = (idx >> 2) % CW, y = idx / (4 * CW);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + y < H && col0 + xx < W) v = *reinterpret_cast<const float4*>(dz + (((size_t)crop * H + row0 + y) * W + col0 + xx) * 16 + q * 4);
        reinterpret_cast<float4*>(ds)[idx] = v;
    }
    __syncthreads();
    const int co = tid & 15, ky = (tid >> 4) % TAPS, g = tid / (16 * TAPS);
    float acc[CH][TAPS];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int k = 0; k < TAPS; ++k) acc[c][k] = 0.f;
    if (tid < ACT) {
#pragma unroll 1
        for (int yy = 0; yy < 2; ++yy) {
            const int y = g * 2 + yy;
            const float* xr = xs + (y + ky) * PW * CH;
            const float* dr = ds + y * CW * 16 + co;
            float win[CH][TAPS];
#pragma unroll
            for (int c = 0; c < CH; ++c)
#pragma unroll
                for (int k = 1; k < TAPS; ++k) win[c][k] = xr[(k - 1) * CH + c];
#pragma unroll 4
            for (int xx = 0; xx < CW; ++xx) {
                const float d = dr[xx * 16];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
#pragma unroll
                    for (int k = 0; k < TAPS - 1; ++k) win[c][k] = win[c][k + 1];
                    win[c][TAPS - 1] = xr[(xx + TAPS - 1) * CH + c];
#pragma unroll
                    for (int k = 0; k < TAPS; ++k) acc[c][k] += win[c][k] * d;
                }
            }
        }
    }
    __syncthreads();                                                   // ds becomes the row pairs' exchange: [g][c][tap][co]
    if (tid < ACT)
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int k = 0; k < TAPS; ++k) ds[((g * CH + c) * T2 + ky * TAPS + k) * 16 + co] = acc[c][k];
    __syncthreads();
    if (tid >= TW) return;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        part[(size_t)blockIdx.x * CH * TW + c * TW + tid] = ((ds[c * TW + tid] + ds[(CH + c) * TW + tid]) + ds[(2 * CH + c) * TW + tid]) + ds[(3 * CH + c) * TW + tid];
}

// ------------------------------------------------------------------------------------------------
// BN (batch statistics) + ReLU + floor 2x2 max-pool + dropout (per channel, or per element: ELEM) on a plane of H x W pixels: z [n][H][W][C] -> a [n][H/2][W/2][C].
// The odd last row / column is read by no window
// ------------------------------------------------------------------------------------------------
template <int C>
__device__ __forceinline__ void load_window_hw(const float* __restrict__ z, int H, int W, int crop, int py, int px, int c4, float4 v[4]) {
    const float* base = z + (((size_t)crop * H + 2 * py) * W + 2 * px) * C + c4 * 4;
    v[0] = *reinterpret_cast<const float4*>(base);
    v[1] = *reinterpret_cast<const float4*>(base + C);
    v[2] = *reinterpret_cast<const float4*>(base + (size_t)W * C);
    v[3] = *reinterpret_cast<const float4*>(base + (size_t)W * C + C);
}

// Where the keep bytes lie.  ELEM = false: Dropout2d, one byte per (crop, channel), keep [n][C].  ELEM = true (the category network, nn.Dropout on
// the pooled plane): one byte per pooled element, keep [n][H/2][W/2][creal] with creal % 4 == 0, so a lane's four channels are one aligned 32-bit
// load; a lane whose channels are >= creal (block 3: 100 real channels in 128 slots) reads nothing and is closed whatever its slots hold -- its
// activation and every gradient through it are 0, the padding argument of train_arch.hip
__device__ __forceinline__ uint32_t elem_keep_word(const uint8_t* __restrict__ keep, const int creal, const size_t pos, const int c4) {
    return c4 * 4 < creal ? *reinterpret_cast<const uint32_t*>(keep + pos * creal + c4 * 4) : 0u;
}
template <int C, bool ELEM>
__device__ __forceinline__ bool is_kept(const uint8_t* __restrict__ keep, const uint32_t word, const int crop, const int c4, const int k) {
    if (ELEM) return ((word >> (8 * k)) & 0xffu) != 0;
    return keep[(size_t)crop * C + c4 * 4 + k] != 0;
}

template <int C, bool ELEM = false>
__global__ __launch_bounds__(256) void k_tany_bn_pool(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                      const float* __restrict__ g, const float* __restrict__ be, const uint8_t* __restrict__ keep /*[n][C]*/,
                                                      float scale, float* __restrict__ a, int n, int H, int W, int creal) {
    const int Hp = H / 2, Wp = W / 2;
    const size_t total = (size_t)n * Hp * Wp * (C / 4);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c4 = idx % (C / 4);
    const size_t pos = idx / (C / 4);
    const int px = pos % Wp, py = (pos / Wp) % Hp, crop = pos / ((size_t)Hp * Wp);
    float4 v[4];
    load_window_hw<C>(z, H, W, crop, py, px, c4, v);
    const uint32_t kw = ELEM ? elem_keep_word(keep, creal, pos, c4) : 0u;
    float4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c4 * 4 + k;
        const float alpha = invstd[c] * g[c], beta = be[c] - mean[c] * alpha;
        float m = f4get(v[0], k) * alpha + beta;
#pragma unroll
        for (int q = 1; q < 4; ++q) m = fmaxf(m, f4get(v[q], k) * alpha + beta);
        m = fmaxf(m, 0.f);
        f4set(out, k, is_kept<C, ELEM>(keep, kw, crop, c4, k) ? m * scale : 0.f);
    }
    *reinterpret_cast<float4*>(a + pos * C + c4 * 4) = out;
}

// sums of dy and dy * x-hat per channel (BN backward) from the pooled gradient: partial[block][2][C] (FIN_BN_BWD).
// dy is non-zero at the arg-max of a pool window only, so the pixels outside every window add nothing here -- they do count in the
// 1 / (n H W) of the means (train.hip: bn_backward)
template <int C, bool ELEM = false>
__global__ __launch_bounds__(256) void k_tany_pool_bwd_stats(const float* __restrict__ da, const float* __restrict__ z, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, const float* __restrict__ g, const float* __restrict__ be,
                                                             const uint8_t* __restrict__ keep, float scale, int n, int H, int W, double* __restrict__ partial, int creal) {
    constexpr int LC = C / 4, RL = 256 / LC;
    __shared__ double sh[RL * C];
    const int tid = threadIdx.x, cl = tid % LC, rl = tid / LC;
    const int Hp = H / 2, Wp = W / 2;
    const size_t rows = (size_t)n * Hp * Wp;
    float mn[4], iv[4], al[4], bt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = cl * 4 + k;
        mn[k] = mean[c]; iv[k] = invstd[c]; al[k] = iv[k] * g[c]; bt[k] = be[c] - mn[k] * al[k];
    }
    double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    for (size_t r = (size_t)blockIdx.x * RL + rl; r < rows; r += (size_t)gridDim.x * RL) {
        const int px = r % Wp, py = (r / Wp) % Hp, crop = r / ((size_t)Hp * Wp);
        float4 v[4];
        load_window_hw<C>(z, H, W, crop, py, px, cl, v);
        const float4 d = *reinterpret_cast<const float4*>(da + r * C + cl * 4);
        const uint32_t kw = ELEM ? elem_keep_word(keep, creal, r, cl) : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float zq[4] = {f4get(v[0], k), f4get(v[1], k), f4get(v[2], k), f4get(v[3], k)};
            int arg; float xh;
            const float gy = pooled_grad(zq, mn[k], iv[k], al[k], bt[k], f4get(d, k), is_kept<C, ELEM>(keep, kw, crop, cl, k), scale, &arg, &xh);
            acc[0][k] += gy; acc[1][k] += (double)gy * xh;
        }
    }
    block_columns<C, 2>(acc, sh, partial);
}

// dz = gamma * invstd * (dy - mean(dy) - x-hat * mean(dy x-hat)) written over z (dy is non-zero at the pool's arg-max only); the column sums of what
// was written are the convolution bias's gradient (rounding noise around 0: the bias feeds a BatchNorm): partial[block][1][C] (FIN_BIAS).  The walk is over ceil(H/2) x ceil(W/2) windows: a window past the pooled plane
// (odd H or W) has no arg-max and no dy, but its pixels inside the image still get dz = gamma invstd (0 - mean(dy) - x-hat mean(dy x-hat)),
// which the weight gradient, the data gradient and the bias sum below all see.  A thread's elements lie a grid-stride apart (a multiple of
// C / 4: it stays on its four channels)
template <int C, bool ELEM = false>
__global__ __launch_bounds__(256) void k_tany_bn_bwd(const float* __restrict__ da, float* __restrict__ z, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ g, const float* __restrict__ be,
                                                     const uint8_t* __restrict__ keep, float scale, const float* __restrict__ sums, float inv_count, int n, int H,
                                                     int W, double* __restrict__ partial, int creal) {
    constexpr int LC = C / 4, RL = 256 / LC;
    __shared__ double sh[RL * C];
    const int Hp = H / 2, Wp = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
    const size_t total = (size_t)n * Hc * Wc * LC;
    const int c4 = threadIdx.x % LC;
    float mn[4], iv[4], al[4], bt[4], m1[4], m2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c4 * 4 + k;
        mn[k] = mean[c]; iv[k] = invstd[c]; al[k] = iv[k] * g[c]; bt[k] = be[c] - mn[k] * al[k];
        m1[k] = sums[c] * inv_count; m2[k] = sums[C + c] * inv_count;
    }
    double acc[1][4] = {{0, 0, 0, 0}};
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const size_t pos = idx / LC;
        const int px = pos % Wc, py = (pos / Wc) % Hc, crop = pos / ((size_t)Hc * Wc);
        const bool pooled = py < Hp && px < Wp;                         // all four pixels exist and the pool has an output here
        const bool vq[4] = {true, 2 * px + 1 < W, 2 * py + 1 < H, 2 * px + 1 < W && 2 * py + 1 < H};
        float* base = z + (((size_t)crop * H + 2 * py) * W + 2 * px) * C + c4 * 4;
        const size_t qoff[4] = {0, (size_t)C, (size_t)W * C, (size_t)W * C + C};
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = vq[q] ? *reinterpret_cast<const float4*>(base + qoff[q]) : make_float4(0.f, 0.f, 0.f, 0.f);
        const size_t pr = ((size_t)crop * Hp + py) * Wp + px;             // the pooled element, where there is one
        const float4 d = pooled ? *reinterpret_cast<const float4*>(da + pr * C + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const uint32_t kw = ELEM && pooled ? elem_keep_word(keep, creal, pr, c4) : 0u;
        float4 o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float zq[4] = {f4get(v[0], k), f4get(v[1], k), f4get(v[2], k), f4get(v[3], k)};
            int arg = -1; float xh;
            float gy = 0.f;
            if (pooled) gy = pooled_grad(zq, mn[k], iv[k], al[k], bt[k], f4get(d, k), is_kept<C, ELEM>(keep, kw, crop, c4, k), scale, &arg, &xh);
            float wsum = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float xhat = (zq[q] - mn[k]) * iv[k];
                float dzv = al[k] * ((q == arg ? gy : 0.f) - m1[k] - xhat * m2[k]);
                if (ELEM && c4 * 4 + k >= creal) dzv = 0.f;                 // a padded channel: 0 whatever its slots hold
                f4set(o[q], k, dzv);
                if (vq[q]) wsum += dzv;
            }
            acc[0][k] += wsum;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (vq[q]) *reinterpret_cast<float4*>(base + qoff[q]) = o[q];
    }
    block_columns<C, 1>(acc, sh, partial);
}

// ------------------------------------------------------------------------------------------------
// fc1 at P = (H/8)(W/8) positions (run time, 1..1024; 100 at 80x80).  h[n][100] = a3[n][p][c] . W1c[p][c][o]: one partial plane per position,
// added in position order by k_tany_fc1_sum (at 80x80 by the head kernel) -- an order that depends on the size and never on n.
// Block = one position x 64 samples on fp32 MFMA (32x32x2: one step contracts two channels); wave = 32 outputs (the last wave: 4), two sample
// tiles.  (The VALU form -- 8 x 4 outputs per thread, 12 LDS reads per 32 multiply-adds, one wave per SIMD -- took 30 us at 80x80.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tany_fc1(const float* __restrict__ a3 /*[n][P][128]*/, const float* __restrict__ w /*[P][128][100]*/,
                                                  float* __restrict__ hpart /*[P][n][100]*/, int n, int P) {
    __shared__ float As[64 * 129];                                    // [sample][channel], pitch 129: the 32 rows of a fragment on 32 banks
    __shared__ __attribute__((aligned(16))) float Ws[128 * 100];      // [channel][output]
    const int tid = threadIdx.x, hw = blockIdx.x, n0 = blockIdx.y * 64;
    for (int idx = tid; idx < 64 * 32; idx += 256) {
        const int i = idx >> 5, q = idx & 31;
        const float4 v = (n0 + i < n) ? *reinterpret_cast<const float4*>(a3 + ((size_t)(n0 + i) * P + hw) * 128 + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        float* d = As + i * 129 + q * 4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    {
        const float4* src = reinterpret_cast<const float4*>(w + (size_t)hw * 12800);
        for (int idx = tid; idx < 3200; idx += 256) reinterpret_cast<float4*>(Ws)[idx] = src[idx];
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int o = wave * 32 + j;
    const bool ov = o < 100;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const float* a0 = As + j * 129 + h;
    const float* a1 = As + (32 + j) * 129 + h;
    const float* bp = Ws + h * 100 + (ov ? o : 0);
#pragma unroll 8
    for (int t = 0; t < 64; ++t) {
        const float bv = ov ? bp[2 * t * 100] : 0.f;
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[2 * t], bv, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[2 * t], bv, acc1, 0, 0, 0);
    }
    if (!ov) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * h;                 // accumulator r of lane (j, h) is row 8 (r / 4) + 4 h + r % 4
        if (n0 + i < n) hpart[((size_t)hw * n + n0 + i) * 100 + o] = acc0[r];
        if (n0 + 32 + i < n) hpart[((size_t)hw * n + n0 + 32 + i) * 100 + o] = acc1[r];
    }
}

// hsum[n][100] = hpart[0] + hpart[1] + ... + hpart[P - 1], in that order (eight loads in flight)
__global__ __launch_bounds__(256) void k_tany_fc1_sum(const float* __restrict__ hpart, int count /*n * 100*/, int P, float* __restrict__ hsum) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    float acc = 0.f;
    for (int p0 = 0; p0 < P; p0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p0 + k < P ? hpart[(size_t)(p0 + k) * count + idx] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) if (p0 + k < P) acc += v[k];
    }
    hsum[idx] = acc;
}

// dW1c[p][c][o] = sum_n a3[n][p][c] * dh[n][o]: block = one position, wave = 32 channels x all outputs, samples in order
__global__ __launch_bounds__(256) void k_tany_fc1_wgrad(const float* __restrict__ a3, const float* __restrict__ dh, float* __restrict__ gw, int n, int P) {
    const int tid = threadIdx.x, lane = tid & 63, mt = tid >> 6, j = lane & 31, h = lane >> 5, hw = blockIdx.x;
    f32x16 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    const float* ap = a3 + (size_t)hw * 128 + mt * 32 + j;
    const size_t sstride = (size_t)P * 128;
    const bool last_ok = 96 + j < 100;
    for (int s0 = 0; s0 < n; s0 += 2) {
        const int s = s0 + h;
        const bool ok = s < n;
        const float av = ok ? ap[(size_t)s * sstride] : 0.f;
        float bv[4];
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) bv[nt] = ok ? dh[(size_t)s * 100 + nt * 32 + j] : 0.f;
        bv[3] = (ok && last_ok) ? dh[(size_t)s * 100 + 96 + j] : 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[nt], acc[nt], 0, 0, 0);
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int o = nt * 32 + j;
        if (o >= 100) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = mt * 32 + 8 * (r / 4) + 4 * h + (r % 4);
            gw[((size_t)hw * 128 + c) * 100 + o] = acc[nt][r];
        }
    }
}

// da3[n][p][c] = sum_o dh[n][o] * W1c[p][c][o]: block = one position x 32 samples, wave = 32 channels
__global__ __launch_bounds__(256) void k_tany_fc1_dgrad(const float* __restrict__ dh, const float* __restrict__ w, float* __restrict__ da3, int n, int P) {
    __shared__ float Ws[128 * 101];                                   // [channel][output], pitch 101: a fragment's 32 channels on 32 banks
    __shared__ float Ds[32 * 101];                                    // [sample][output]
    const int tid = threadIdx.x, hw = blockIdx.x, n0 = blockIdx.y * 32;
    for (int idx = tid; idx < 128 * 100; idx += 256) Ws[(idx / 100) * 101 + idx % 100] = w[(size_t)hw * 12800 + idx];
    for (int idx = tid; idx < 32 * 100; idx += 256) Ds[(idx / 100) * 101 + idx % 100] = (n0 + idx / 100) < n ? dh[(size_t)n0 * 100 + idx] : 0.f;
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;
    const int c = wave * 32 + j;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* ap = Ds + j * 101 + h;
    const float* bp = Ws + c * 101 + h;
#pragma unroll 10
    for (int t = 0; t < 50; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * t], bp[2 * t], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int nn = n0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (nn < n) da3[((size_t)nn * P + hw) * 128 + c] = acc[r];
    }
}

// the convolution instances, each stated once with its LDS size: [layer - 1] forward, data gradient
struct ConvInst {
    void (*fn)(const float*, const float*, const float*, float*, int, int, int, int, int);
    int lds;
};
const ConvInst CONV_FWD[2] = {{&k_tany_conv<16, 64, 16, 64>, TanyGeom<64, 16>::LDS_BYTES}, {&k_tany_conv<64, 128, 32, 128>, TanyGeom<128, 32>::LDS_BYTES}};
// conv2's data gradient has 16 output channels: a 32-wide tile, half of it padding, as in the 80x80 fp16 path
const ConvInst CONV_DGRAD[2] = {{&k_tany_conv<64, 32, 16, 16>, TanyGeom<32, 16>::LDS_BYTES}, {&k_tany_conv<128, 64, 32, 64>, TanyGeom<64, 32>::LDS_BYTES}};
// the same four at 3 taps (the category network): the tiles, the LDS layout and the register layout are the 5-tap ones, the patch is smaller
const ConvInst CONV_FWD3[2] = {{&k_tany_conv<16, 64, 16, 64, 3>, TanyGeom<64, 16>::LDS_BYTES}, {&k_tany_conv<64, 128, 32, 128, 3>, TanyGeom<128, 32>::LDS_BYTES}};
const ConvInst CONV_DGRAD3[2] = {{&k_tany_conv<64, 32, 16, 16, 3>, TanyGeom<32, 16>::LDS_BYTES}, {&k_tany_conv<128, 64, 32, 64, 3>, TanyGeom<64, 32>::LDS_BYTES}};

void launch_conv(hipStream_t s, const ConvInst& k, const TrainAnyLayer& L, int n, const float* in, const float* w, const float* bias, float* out) {
    hipLaunchKernelGGL(k.fn, dim3((unsigned)n * L.tiles.tiles), dim3(512), k.lds, s, in, w, bias, out, L.h, L.w, L.tiles.TX, L.tiles.tx_n, L.tiles.tiles);
}

}  // namespace

int tany_attrs() {
    for (const ConvInst* set : {CONV_FWD, CONV_DGRAD, CONV_FWD3, CONV_DGRAD3})
        for (int i = 0; i < 2; ++i)
            TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(set[i].fn), hipFuncAttributeMaxDynamicSharedMemorySize, set[i].lds));
    return TREXHIP_OK;
}

void tany_conv1(hipStream_t s, const TrainAnyGeom& g, int n, const float* x, const float* w, const float* b, float* z) {
    // the 3-tap chain is the category network's: its conv1 pair normalises the input (tany_input)
    const auto fn = g.taps == 3 ? (g.CH == 1 ? &k_tany_conv1<1, 3, true> : &k_tany_conv1<3, 3, true>) : (g.CH == 1 ? &k_tany_conv1<1> : &k_tany_conv1<3>);
    hipLaunchKernelGGL(fn, dim3((unsigned)n * g.c1_tiles), dim3(256), 0, s, x, w, b, z, g.W, g.H, g.c1_tx, g.c1_tiles);
}

void tany_conv_fwd(hipStream_t s, const TrainAnyGeom& g, int layer, int n, const float* in, const float* w, const float* bias, float* z) {
    launch_conv(s, (g.taps == 3 ? CONV_FWD3 : CONV_FWD)[layer - 1], g.L[layer], n, in, w, bias, z);
}

void tany_conv_dgrad(hipStream_t s, const TrainAnyGeom& g, int layer, int n, const float* dz, const float* wb, float* da) {
    launch_conv(s, (g.taps == 3 ? CONV_DGRAD3 : CONV_DGRAD)[layer - 1], g.L[layer], n, dz, wb, nullptr, da);
}

void tany_wgrad(hipStream_t s, const TrainAnyGeom& g, int layer, int n, const float* a, const float* dz, float* part) {
    const TrainAnyLayer& L = g.L[layer];
    const dim3 grid(L.wg_types, g.wg_shares(layer, n));
    const int rows = n * L.h, per = g.wg_per(layer, n);
    if (g.taps == 3) {
        if (layer == 1) hipLaunchKernelGGL((k_tany_wgrad<16, 64, 3>), grid, dim3(TanyWgradGeom<16, 3>::NW * 64), 0, s, a, dz, part, rows, per, L.h, L.w);
        else hipLaunchKernelGGL((k_tany_wgrad<64, 128, 3>), grid, dim3(TanyWgradGeom<64, 3>::NW * 64), 0, s, a, dz, part, rows, per, L.h, L.w);
        return;
    }
    if (layer == 1) hipLaunchKernelGGL((k_tany_wgrad<16, 64>), grid, dim3(TanyWgradGeom<16>::NW * 64), 0, s, a, dz, part, rows, per, L.h, L.w);
    else hipLaunchKernelGGL((k_tany_wgrad<64, 128>), grid, dim3(TanyWgradGeom<64>::NW * 64), 0, s, a, dz, part, rows, per, L.h, L.w);
}

void tany_wgrad1(hipStream_t s, const TrainAnyGeom& g, int n, const float* x, const float* dz, float* part) {
    const auto fn = g.taps == 3 ? (g.CH == 1 ? &k_tany_wgrad1<1, 3, true> : &k_tany_wgrad1<3, 3, true>) : (g.CH == 1 ? &k_tany_wgrad1<1> : &k_tany_wgrad1<3>);
    hipLaunchKernelGGL(fn, dim3((unsigned)n * g.wg1_tiles), dim3(512), 0, s, x, dz, part, g.W, g.H, g.wg1_tx, g.wg1_tiles);
}

// creal = 0: channel masks [n][C]; creal > 0: element masks [n][h/2][w/2][creal], channels >= creal closed (is_kept)
void tany_bn_pool(hipStream_t s, int C, const float* z, const float* mean, const float* invstd, const float* g, const float* be, const uint8_t* keep, float scale,
                  float* a, int n, int h, int w, int creal) {
    const size_t total = (size_t)n * (h / 2) * (w / 2) * (C / 4);
    const auto fn = creal ? (C == 16 ? &k_tany_bn_pool<16, true> : C == 64 ? &k_tany_bn_pool<64, true> : &k_tany_bn_pool<128, true>)
                          : (C == 16 ? &k_tany_bn_pool<16> : C == 64 ? &k_tany_bn_pool<64> : &k_tany_bn_pool<128>);
    hipLaunchKernelGGL(fn, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, z, mean, invstd, g, be, keep, scale, a, n, h, w, creal);
}

void tany_pool_bwd_stats(hipStream_t s, int C, int blocks, const float* da, const float* z, const float* mean, const float* invstd, const float* g, const float* be,
                         const uint8_t* keep, float scale, int n, int h, int w, double* partial, int creal) {
    const auto fn = creal ? (C == 16 ? &k_tany_pool_bwd_stats<16, true> : C == 64 ? &k_tany_pool_bwd_stats<64, true> : &k_tany_pool_bwd_stats<128, true>)
                          : (C == 16 ? &k_tany_pool_bwd_stats<16> : C == 64 ? &k_tany_pool_bwd_stats<64> : &k_tany_pool_bwd_stats<128>);
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), 0, s, da, z, mean, invstd, g, be, keep, scale, n, h, w, partial, creal);
}

int tany_bn_bwd(hipStream_t s, int C, int max_blocks, const float* da, float* z, const float* mean, const float* invstd, const float* g, const float* be,
                const uint8_t* keep, float scale, const float* sums, float inv_count, int n, int h, int w, double* partial, int creal) {
    const size_t total = (size_t)n * ((h + 1) / 2) * ((w + 1) / 2) * (C / 4);
    // whole rounds, as at 80x80: every workgroup takes the same number of elements
    const size_t nb0 = (total + 255) / 256, per = (nb0 + max_blocks - 1) / max_blocks, nb = (nb0 + per - 1) / per;
    const auto fn = creal ? (C == 16 ? &k_tany_bn_bwd<16, true> : C == 64 ? &k_tany_bn_bwd<64, true> : &k_tany_bn_bwd<128, true>)
                          : (C == 16 ? &k_tany_bn_bwd<16> : C == 64 ? &k_tany_bn_bwd<64> : &k_tany_bn_bwd<128>);
    hipLaunchKernelGGL(fn, dim3((unsigned)nb), dim3(256), 0, s, da, z, mean, invstd, g, be, keep, scale, sums, inv_count, n, h, w, partial, creal);
    return (int)nb;
}

void tany_fc1(hipStream_t s, const TrainAnyGeom& g, int n, const float* a3, const float* w, float* hpart, float* hsum) {
    hipLaunchKernelGGL(k_tany_fc1, dim3(g.P, (n + 63) / 64), dim3(256), 0, s, a3, w, hpart, n, g.P);
    if (hsum) hipLaunchKernelGGL(k_tany_fc1_sum, dim3((n * TA_HID + 255) / 256), dim3(256), 0, s, hpart, n * TA_HID, g.P, hsum);
}

void tany_fc1_wgrad(hipStream_t s, const TrainAnyGeom& g, int n, const float* a3, const float* dh, float* gw) {
    hipLaunchKernelGGL(k_tany_fc1_wgrad, dim3(g.P), dim3(256), 0, s, a3, dh, gw, n, g.P);
}

void tany_fc1_dgrad(hipStream_t s, const TrainAnyGeom& g, int n, const float* dh, const float* w, float* da3) {
    hipLaunchKernelGGL(k_tany_fc1_dgrad, dim3(g.P, (n + 31) / 32), dim3(256), 0, s, dh, w, da3, n, g.P);
}

}  // namespace trexhip
