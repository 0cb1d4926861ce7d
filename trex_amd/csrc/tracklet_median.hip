// tracklet_median.hip -- the pixel-wise median image of every tracklet's crops, on a crop pool that is already in HBM.
//
// Replaces, for fixed-size uint8 crops [n][H][W][C] (what the three crop calls write) and one tracklet per row:
//   hist_utils::init / addImage, Application/src/tracker/ui/Export.cpp:78-154 -- per pixel a histogram of 256 `short` bins and a count; after
//       every image n = count / 2 and `for (i = 0; i < 256 && ((n -= h[i]) >= 0); ++i);`, med = uchar(i) (:104-110)
//   the loop over a tracklet's images, Export.cpp:1287-1364 -- a 1-channel image as it is, a 3-channel one through cv::COLOR_BGR2GRAY
//       (:1320-1327), addImage per image (:1334); only the value after the last image survives (:1355-1361)
// That value is the smallest i whose cumulative count exceeds count / 2 = sorted[count / 2], the upper median at an even count; it does not
// depend on the order of the images.  Bins are `short`: more than 32767 images in a tracklet are refused (undefined in the reference).
//
// Three launches, one look at two flag words, two launches:
//   k_med_count   rows per tracklet with integer atomics + the flag for an id outside [-1, T)                      } the checked pass: writes
//   k_med_scan    exclusive scan of the counts: where a tracklet's rows go in the row list; the lowest tracklet    } scratch only; the host reads
//                 with more than 32767 rows goes into the second flag word                                         } the flags before going on
//   k_med_fill    every row takes the next free place of its tracklet's list (an atomic cursor: the order inside a list does not matter here)
//   k_med_select  one workgroup per (tracklet, tile of 256 gray pixels), a lane owns 4 adjacent pixels: one dword of every listed crop at C = 1,
//                 three at C = 3 (reduced with 24-bit multiplies), so a wave reads 256 (768) contiguous bytes per crop, MED_UNROLL crops in flight.
//                 The four waves of a workgroup split the list.  No 256 bins per pixel: two nibble passes, 16 counters per pixel each, two
//                 counters to a dword (none exceeds 32767, so no carry), indexed with compile-time indices only -- 8 compare-select-adds per
//                 byte and pass.  Pass A counts the high nibbles; the waves' counters are added in LDS (integer adds: order-free); every wave
//                 picks the nibble that holds rank rows / 2 and the rank left inside it.  Pass B re-reads the tile (L2) and counts the low
//                 nibbles of the bytes whose high nibble matches.  Where the pool's base, the crop size and the output allow, loads and the
//                 store are dwords; otherwise the same kernel runs on bytes.
// Reads n*H*W*C bytes from HBM once and writes T*H*W; bounded by issue (about 50 lane operations per input byte), not by bandwidth.
#include "internal.h"
#include <algorithm>
#include <cstring>
#include <string>

namespace trexhip {
namespace {

constexpr int MED_THREADS = 256, MED_WAVES = MED_THREADS / 64, MED_TILE = 256, MED_UNROLL = 4;
constexpr int MED_MAX_ROWS = 32767;                    // Hist::h is vector<short> (Export.cpp:85-89)
constexpr int MED_MAX_N = 1 << 24, MED_MAX_T = 1 << 24, MED_MIN_SIDE = 8, MED_MAX_SIDE = 256;
constexpr unsigned MED_MAX_GRID = 1u << 20;

struct MedArgs {
    const uint8_t* crops; int n, HW, C;
    const int32_t* tracklet; int T;
    uint32_t* flag;                  // [0] an id outside [-1, T); [1] the lowest tracklet with more than MED_MAX_ROWS rows, or ~0
    uint32_t* cnt;                   // [T] rows of every tracklet
    uint32_t* offs;                  // [T] exclusive scan of cnt
    uint32_t* cursor;                // [T] places of a tracklet's list that are taken
    int32_t* list;                   // [n] row indices grouped by tracklet
    uint8_t* median;                 // [T][HW]
};

__global__ __launch_bounds__(MED_THREADS) void k_med_count(const MedArgs A) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * MED_THREADS + threadIdx.x; i < (size_t)A.n; i += (size_t)gridDim.x * MED_THREADS) {
        const int32_t t = A.tracklet[i];
        if (t < -1 || t >= A.T) bad = true;
        else if (t >= 0) atomicAdd(A.cnt + t, 1u);
    }
    if (bad) atomicOr(A.flag, 1u);
}

// one workgroup: every thread sums a contiguous piece, the pieces are scanned through LDS, every thread writes its piece's exclusive prefixes
__global__ __launch_bounds__(1024) void k_med_scan(const MedArgs A) {
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x, m = A.T, per = (m + 1023) / 1024;
    const int a = (int)min((long long)tid * per, (long long)m), b = min(a + per, m);
    uint32_t sum = 0;
    for (int i = a; i < b; ++i) {
        const uint32_t v = A.cnt[i];
        if (v > (uint32_t)MED_MAX_ROWS) atomicMin(A.flag + 1, (uint32_t)i);
        sum += v;
    }
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int t = 0; t < 1024; ++t) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (int i = a; i < b; ++i) { A.offs[i] = run; run += A.cnt[i]; }
}

__global__ __launch_bounds__(MED_THREADS) void k_med_fill(const MedArgs A) {
    for (size_t i = (size_t)blockIdx.x * MED_THREADS + threadIdx.x; i < (size_t)A.n; i += (size_t)gridDim.x * MED_THREADS) {
        const int32_t t = A.tracklet[i];                               // in [-1, T): the checked pass ran first
        if (t < 0) continue;
        const uint32_t at = atomicAdd(A.cursor + t, 1u);
        if (at < A.cnt[t]) A.list[A.offs[t] + at] = (int32_t)i;        // always, unless d_tracklet changed under the call
    }
}

// the 4 gray bytes of pixels p0..p0+3 of one crop, pixel p in bits 8p..8p+7; 0 for a pixel behind the crop's last
template <int C, bool DW>
__device__ __forceinline__ uint32_t med_load(const uint8_t* __restrict__ crop, const int p0, const int HW) {
    if constexpr (DW) {                                                // HW % 4 == 0: the lane's 4 pixels are all inside or all outside
        if (p0 >= HW) return 0u;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(crop + (size_t)p0 * C);
        if constexpr (C == 1) return src[0];
        uint32_t w[3] = {src[0], src[1], src[2]}, out = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            uint32_t c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int byte = p * 3 + k;
                c[k] = (w[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
            }
            out |= ((__umul24(c[0], 1868u) + __umul24(c[1], 9617u) + __umul24(c[2], 4899u) + 8192u) >> 14) << (8 * p);   // cv::COLOR_BGR2GRAY on B, G, R bytes
        }
        return out;
    } else {
        uint32_t out = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (p0 + p >= HW) break;
            const uint8_t* px = crop + (size_t)(p0 + p) * C;
            uint32_t g;
            if constexpr (C == 1) g = px[0];
            else g = (__umul24((uint32_t)px[0], 1868u) + __umul24((uint32_t)px[1], 9617u) + __umul24((uint32_t)px[2], 4899u) + 8192u) >> 14;
            out |= g << (8 * p);
        }
        return out;
    }
}

// counters of one pixel: dword k holds nibble 2k in its low and nibble 2k + 1 in its high half
__device__ __forceinline__ void med_add(uint32_t (&c)[8], const uint32_t nibble, const uint32_t one) {
    const uint32_t inc = one << ((nibble & 1u) * 16u), j = nibble >> 1;
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] += j == (uint32_t)k ? inc : 0u;
}

// PASS 0: every byte's high nibble; PASS 1: the low nibble of the bytes whose high nibble is hi[p]
template <int PASS>
__device__ __forceinline__ void med_take(uint32_t (&c)[4][8], const uint32_t g, const uint32_t (&hi)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t v = (g >> (8 * p)) & 0xffu;
        if constexpr (PASS == 0) med_add(c[p], v >> 4, 1u);
        else med_add(c[p], v & 15u, (v >> 4) == hi[p] ? 1u : 0u);
    }
}

template <int C, bool DW, int PASS>
__device__ __forceinline__ void med_pass(const MedArgs& A, const int32_t* __restrict__ lst, const int rows, const int wave, const int p0,
                                         const uint32_t (&hi)[4], uint32_t (&c)[4][8]) {
    const size_t per = (size_t)A.HW * C;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 8; ++k) c[p][k] = 0u;
    int i = wave;                                                      // wave-uniform: list entries wave, wave + MED_WAVES, ...
    for (; i + (MED_UNROLL - 1) * MED_WAVES < rows; i += MED_UNROLL * MED_WAVES) {
        uint32_t g[MED_UNROLL];
#pragma unroll
        for (int u = 0; u < MED_UNROLL; ++u) g[u] = med_load<C, DW>(A.crops + (size_t)lst[i + u * MED_WAVES] * per, p0, A.HW);
#pragma unroll
        for (int u = 0; u < MED_UNROLL; ++u) med_take<PASS>(c, g[u], hi);
    }
    for (; i < rows; i += MED_WAVES) med_take<PASS>(c, med_load<C, DW>(A.crops + (size_t)lst[i] * per, p0, A.HW), hi);
}

// the waves' counters into the workgroup's (s[q][lane]: a wave's 64 lanes hit 64 banks), then everyone reads the sums
__device__ __forceinline__ void med_reduce(uint32_t (*s)[64], const int lane, uint32_t (&c)[4][8], const bool single) {
    if (single) return;                                                // rows <= 1 wave's share: wave 0 holds everything (block-uniform)
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c[p][k]) atomicAdd(&s[p * 8 + k][lane], c[p][k]);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 8; ++k) c[p][k] = s[p * 8 + k][lane];
}

// the walk `for (i = 0; i < 16 && ((n -= h[i]) >= 0); ++i)` over one pixel's 16 counters: the nibble that holds rank n and the rank left in it
__device__ __forceinline__ void med_walk(const uint32_t (&c)[8], uint32_t& rank, uint32_t& nibble) {
    bool done = false;
    nibble = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t h = (c[k >> 1] >> (16 * (k & 1))) & 0xffffu;
        const bool here = !done && rank < h;
        if (here) nibble = (uint32_t)k;
        done |= here;
        if (!done) rank -= h;
    }
}

// four waves per SIMD: without the hint the scheduler spends 130 VGPRs on the unrolled compare-select-adds, two over the step to three waves
template <int C, bool DW>
__global__ __launch_bounds__(MED_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void k_med_select(const MedArgs A, const int tiles, const unsigned long long items) {
    __shared__ uint32_t s_a[32][64], s_b[32][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (unsigned long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int t = (int)(item / (unsigned)tiles), tile = (int)(item % (unsigned)tiles);
        const int rows = (int)A.cnt[t], p0 = tile * MED_TILE + lane * 4;
        const bool single = rows <= 1;
        uint32_t out = 0u;
        if (rows > 0) {
            if (!single) {
                __syncthreads();                                       // the last item's sums have been read
                for (int q = threadIdx.x; q < 32 * 64; q += MED_THREADS) { (&s_a[0][0])[q] = 0u; (&s_b[0][0])[q] = 0u; }
                __syncthreads();
            }
            const int32_t* lst = A.list + A.offs[t];
            uint32_t c[4][8], hi[4] = {0u, 0u, 0u, 0u}, rank[4];
            med_pass<C, DW, 0>(A, lst, rows, wave, p0, hi, c);
            med_reduce(s_a, lane, c, single);
#pragma unroll
            for (int p = 0; p < 4; ++p) { rank[p] = (uint32_t)rows / 2u; med_walk(c[p], rank[p], hi[p]); }
            med_pass<C, DW, 1>(A, lst, rows, wave, p0, hi, c);
            med_reduce(s_b, lane, c, single);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                uint32_t lo;
                med_walk(c[p], rank[p], lo);
                out |= (hi[p] << 4 | lo) << (8 * p);
            }
        }
        if (wave != 0) continue;                                       // every wave holds the same bytes (at rows <= 1 only wave 0 does)
        uint8_t* dst = A.median + (size_t)t * A.HW;
        if constexpr (DW) {
            if (p0 < A.HW) *reinterpret_cast<uint32_t*>(dst + p0) = out;
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (p0 + p < A.HW) dst[p0 + p] = (uint8_t)(out >> (8 * p));
        }
    }
}

size_t med_up16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace
}  // namespace trexhip

using namespace trexhip;

extern "C" {

int trexhip_tracklet_medians_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n, int32_t width, int32_t height, int32_t channels,
                                    const int32_t* d_tracklet, int32_t n_tracklets, uint8_t* d_median, uint32_t* d_rows) {
    const std::string who = "trexhip_tracklet_medians_device";
    if (!ctx) { set_error(who + ": null context"); return TREXHIP_E_INVALID; }
    if (width < MED_MIN_SIDE || width > MED_MAX_SIDE || height < MED_MIN_SIDE || height > MED_MAX_SIDE) {
        set_error(who + ": width and height must be 8..256 (individual_image_size)");
        return TREXHIP_E_UNSUPPORTED;
    }
    if (channels != 1 && channels != 3) { set_error(who + ": channels must be 1 or 3 (Export.cpp:1322-1328)"); return TREXHIP_E_UNSUPPORTED; }
    if (n < 0 || n > MED_MAX_N) { set_error(who + ": n must be 0..2^24"); return TREXHIP_E_INVALID; }
    if (n_tracklets < 1 || n_tracklets > MED_MAX_T) { set_error(who + ": n_tracklets must be 1..2^24"); return TREXHIP_E_INVALID; }
    if (!d_median || !d_rows || (n > 0 && (!d_crops || !d_tracklet))) { set_error(who + ": null argument"); return TREXHIP_E_INVALID; }
    const int T = n_tracklets, HW = width * height;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    if (n == 0) {                                                      // the state hist_utils::init leaves
        TH_CHECK_HIP(hipMemsetAsync(d_rows, 0, (size_t)T * 4, s));
        TH_CHECK_HIP(hipMemsetAsync(d_median, 0, (size_t)T * HW, s));
        return TREXHIP_OK;
    }
    // one scratch buffer: [flag | cnt | cursor | offs | list]; flag, cnt and cursor are zeroed in one go
    const size_t o_flag = 0, o_cnt = 16, o_cursor = o_cnt + med_up16((size_t)T * 4), o_offs = o_cursor + med_up16((size_t)T * 4),
                 o_list = o_offs + med_up16((size_t)T * 4), total = o_list + med_up16((size_t)n * 4);
    if (int rc = ctx->med.reserve(ctx, total, who.c_str())) return rc;
    uint8_t* base = ctx->med.as<uint8_t>();
    TH_CHECK_HIP(hipMemsetAsync(base, 0, o_offs, s));
    TH_CHECK_HIP(hipMemsetAsync(base + 4, 0xff, 4, s));
    MedArgs A{};
    A.crops = d_crops; A.n = n; A.HW = HW; A.C = channels;
    A.tracklet = d_tracklet; A.T = T;
    A.flag = reinterpret_cast<uint32_t*>(base + o_flag);
    A.cnt = reinterpret_cast<uint32_t*>(base + o_cnt);
    A.cursor = reinterpret_cast<uint32_t*>(base + o_cursor);
    A.offs = reinterpret_cast<uint32_t*>(base + o_offs);
    A.list = reinterpret_cast<int32_t*>(base + o_list);
    A.median = d_median;
    const int row_grid = std::max(1, std::min(8 * ctx->n_cus, (n + MED_THREADS - 1) / MED_THREADS));
    hipLaunchKernelGGL(k_med_count, dim3(row_grid), dim3(MED_THREADS), 0, s, A);
    hipLaunchKernelGGL(k_med_scan, dim3(1), dim3(1024), 0, s, A);
    TH_CHECK_HIP(hipGetLastError());
    uint32_t flag[2] = {0, 0};
    TH_CHECK_HIP(hipMemcpyAsync(flag, A.flag, 8, hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    if (flag[0]) { set_error(who + ": a tracklet id was outside -1..n_tracklets-1; no output was written"); return TREXHIP_E_INVALID; }
    if (flag[1] != 0xffffffffu) {
        uint32_t count = 0;
        TH_CHECK_HIP(hipMemcpyAsync(&count, A.cnt + flag[1], 4, hipMemcpyDeviceToHost, s));
        TH_CHECK_HIP(hipStreamSynchronize(s));
        set_error(who + ": tracklet " + std::to_string(flag[1]) + " holds " + std::to_string(count) +
                  " rows, more than the 32767 a histogram bin of the reference counts (short, Export.cpp:85-89); no output was written");
        return TREXHIP_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(k_med_fill, dim3(row_grid), dim3(MED_THREADS), 0, s, A);
    const int tiles = (HW + MED_TILE - 1) / MED_TILE;
    const unsigned long long items = (unsigned long long)T * tiles;
    const unsigned grid = (unsigned)std::min<unsigned long long>(items, MED_MAX_GRID);
    const bool dw = HW % 4 == 0 && reinterpret_cast<uintptr_t>(d_crops) % 4 == 0 && reinterpret_cast<uintptr_t>(d_median) % 4 == 0;
    if (channels == 1) {
        if (dw) hipLaunchKernelGGL((k_med_select<1, true>), dim3(grid), dim3(MED_THREADS), 0, s, A, tiles, items);
        else hipLaunchKernelGGL((k_med_select<1, false>), dim3(grid), dim3(MED_THREADS), 0, s, A, tiles, items);
    } else {
        if (dw) hipLaunchKernelGGL((k_med_select<3, true>), dim3(grid), dim3(MED_THREADS), 0, s, A, tiles, items);
        else hipLaunchKernelGGL((k_med_select<3, false>), dim3(grid), dim3(MED_THREADS), 0, s, A, tiles, items);
    }
    TH_CHECK_HIP(hipGetLastError());
    TH_CHECK_HIP(hipMemcpyAsync(d_rows, A.cnt, (size_t)T * 4, hipMemcpyDeviceToDevice, s));
    return TREXHIP_OK;
}

}  // extern "C"
