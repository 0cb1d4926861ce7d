// cnn_skip_kernels.h -- the per-call preparation that lets k_conv12_rs skip passes whose crop rows are all background (the rule: cnn_skip.h).
// Included by cnn.hip inside namespace trexhip.  Four small kernels on the forward pass's stream, no host read between them:
//   k_crop_bands   first / last non-zero row of every crop (it looks at the bytes, not at how the crop was made)
//   k_pass_count   needed passes per block of SKIP_LB consecutive passes
//   k_pass_list    order-preserving compaction of the needed passes into the list k_conv12_rs walks, its length, the entry behind its end
//   k_v3_fill      the V3 rows of every pass that is NOT listed, copied from the V3 image of an all-zero crop (Net::v3e, made at load)
#pragma once

// the words of Net::d_skip
enum : int {
    SK_EMPTY_RANGE = 0,      // the fp16 range flag of the run that made the empty crop's V3 image: non-zero -> every pass is listed
    SK_EMPTY_CTR = 1,        // that run's pass counter
    SK_LEN = 2,              // passes listed by the last call
    SK_NPASS = 3,            // passes of the last call's batch
    SK_FILLED = 4,           // V3 rows the last call filled
    SK_WORDS = 8
};
static constexpr int SKIP_LB = 1024;      // passes per block of the count / list kernels (one per thread)
static constexpr int SKIP_PAD = 1;        // one entry behind the last one: k_conv12_rs clamps every read behind the list's end to it (RS_LIST)
static constexpr int SKIP_FB = 64;        // passes per block of the fill kernel

// one wave per crop: 400 x 16 bytes, unit i lies in row i / 5
__global__ __launch_bounds__(256) void k_crop_bands(const uint8_t* __restrict__ crops, const int n, int2* __restrict__ bands) {
    using G = SkipGeom;
    constexpr int UPR = 80 / 16, UNITS = G::CROP_ROWS * UPR;
    const int lane = threadIdx.x & 63, crop = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (crop >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(crops + (size_t)crop * (G::CROP_ROWS * 80));
    uint4 px[(UNITS + 63) / 64];
#pragma unroll
    for (int k = 0; k < (UNITS + 63) / 64; ++k) {
        const int i = lane + 64 * k;
        px[k] = i < UNITS ? src[i] : make_uint4(0, 0, 0, 0);
    }
    int y0 = G::CROP_ROWS, y1 = -1;
#pragma unroll
    for (int k = 0; k < (UNITS + 63) / 64; ++k) {
        if (px[k].x | px[k].y | px[k].z | px[k].w) {
            const int row = (lane + 64 * k) / UPR;
            y0 = row < y0 ? row : y0;
            y1 = row > y1 ? row : y1;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_xor(y0, d), b = __shfl_xor(y1, d);
        y0 = a < y0 ? a : y0;
        y1 = b > y1 ? b : y1;
    }
    if (lane == 0) bands[crop] = make_int2(y0, y1);
}

struct SkipBandsOf {
    const int2* bands;
    __host__ __device__ SkipBand operator()(const int crop) const { const int2 b = bands[crop]; return {b.x, b.y}; }
};
__device__ __forceinline__ bool skip_needed(const int p, const int total_pairs, const int2* __restrict__ bands, const bool all) {
    return all || skip_pass_needed(p, total_pairs, SkipBandsOf{bands});
}

__global__ __launch_bounds__(SKIP_LB) void k_pass_count(const int2* __restrict__ bands, const int n, const uint32_t* __restrict__ words,
                                                        uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_cnt;
    const int total_pairs = n * SkipGeom::V3_ROWS, n_pass = (total_pairs + SkipGeom::RPP - 1) / SkipGeom::RPP;
    const int p = blockIdx.x * SKIP_LB + threadIdx.x;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const bool need = p < n_pass && skip_needed(p, total_pairs, bands, words[SK_EMPTY_RANGE] != 0);
    const unsigned long long m = __ballot(need);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt, (uint32_t)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt;
}

__global__ __launch_bounds__(SKIP_LB) void k_pass_list(const int2* __restrict__ bands, const int n, uint32_t* __restrict__ words,
                                                       const uint32_t* __restrict__ counts, int* __restrict__ list) {
    __shared__ uint32_t s_base, s_wave[SKIP_LB / 64];
    const int total_pairs = n * SkipGeom::V3_ROWS, n_pass = (total_pairs + SkipGeom::RPP - 1) / SkipGeom::RPP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x * SKIP_LB + tid;
    if (tid == 0) s_base = 0;
    __syncthreads();
    // the needed passes in front of this block
    uint32_t part = 0;
    for (int b = tid; b < (int)blockIdx.x; b += SKIP_LB) part += counts[b];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
    if (lane == 0 && part) atomicAdd(&s_base, part);
    const bool need = p < n_pass && skip_needed(p, total_pairs, bands, words[SK_EMPTY_RANGE] != 0);
    const unsigned long long m = __ballot(need);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = s_base, total = s_base;
    for (int w = 0; w < SKIP_LB / 64; ++w) { const uint32_t c = s_wave[w]; if (w < wave) off += c; total += c; }
    if (need) list[off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = p;
    if (blockIdx.x == gridDim.x - 1) {                                   // the last block knows the length
        if (tid < SKIP_PAD) list[total + tid] = n_pass;
        if (tid == 0) { words[SK_LEN] = total; words[SK_NPASS] = (uint32_t)n_pass; words[SK_FILLED] = 0; }
    }
}

// V3 rows of the passes that are not listed <- the empty crop's rows.  A block looks at SKIP_FB consecutive passes
__global__ __launch_bounds__(256) void k_v3_fill(const int2* __restrict__ bands, const int n, uint32_t* __restrict__ words,
                                                 const uint4* __restrict__ v3e /*[20][V3_ROWB]*/, uint4* __restrict__ v3) {
    using G = SkipGeom;
    static_assert(SKIP_FB == 64, "one ballot");
    __shared__ unsigned long long s_skip;
    constexpr int ROWQ = V3_ROWB / 16;
    const int total_pairs = n * G::V3_ROWS, n_pass = (total_pairs + G::RPP - 1) / G::RPP;
    const int tid = threadIdx.x, p0 = blockIdx.x * SKIP_FB;
    if (tid < 64) {
        const int p = p0 + tid;
        const bool skip = p < n_pass && !skip_needed(p, total_pairs, bands, words[SK_EMPTY_RANGE] != 0);
        const unsigned long long m = __ballot(skip);
        if (tid == 0) s_skip = m;
    }
    __syncthreads();
    unsigned long long m = s_skip;
    uint32_t rows = 0;
    while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int gp0 = (p0 + b) * G::RPP;
        const int nr = total_pairs - gp0 < G::RPP ? total_pairs - gp0 : G::RPP;
        rows += (uint32_t)nr;
        for (int i = tid; i < nr * ROWQ; i += 256) {
            const int r = i / ROWQ, q = i - r * ROWQ;
            const int gp = gp0 + r;
            v3[(size_t)gp * ROWQ + q] = v3e[(gp % G::V3_ROWS) * ROWQ + q];
        }
    }
    if (tid == 0 && rows) atomicAdd(&words[SK_FILLED], rows);
}
