// averages.hip -- the mean probability row per individual of a candidate range, on probabilities and ids that are already in HBM.
//
// Replaces, for softmax rows [n][classes] (trexhip_identify_device's or trexhip_train_predict_device's) and one dense id per row:
//   VINetwork::paverages, Application/src/tracker/ml/VisualIdentification.h:145-180 -- per id the float32 sum of its rows in ascending row
//       order (std::transform(..., std::plus<>{}), :159-175; `float samples; ++samples`, :171), then one division by float(samples) (:177-178)
//   the arg-max scan of Accumulation::check_additional_range, Application/src/tracker/ui/Accumulation.cpp:526-541, over every averaged row:
//       max_p = 0, take index i iff v > max_p -- the first index of the largest entry that is > 0, -1 / 0 for a row without one
//
// A sum over the rows of one (id, class) is ONE chain of dependent float32 additions in row order: it is never split across threads or
// re-associated, so the result equals the host loop bit for bit.  The parallelism is the n_ids x classes independent chains, which makes the
// call latency-bound (a chain is about n / n_ids dependent loads + adds long), not bandwidth-bound.
//
// Four launches, then one copy to the host:
//   k_avg_count   histogram of the ids per (id, segment of rows) with integer atomics + the flag for an id outside 0..n_ids-1
//   k_avg_scan    exclusive scan over the n_ids x segments counts (id-major): where the rows of every (id, segment) go in the row list
//   k_avg_fill    the stable fill: one wave per (id, segment) walks the segment's ids in row order and compacts the matching row indices
//                 with wave ballots and prefix counts -> per id the list of its rows, ascending.  (The rows are cut into segments only so
//                 that an id's list is made by several waves side by side; the list does not depend on the cut.)
//   k_avg_sum     one workgroup per id, lanes along the classes (a row is one coalesced read of 4 x classes bytes, one dword per lane, so
//                 d_probs needs no alignment beyond a float's): walks the id's list AVG_UNROLL rows at a time -- that many independent
//                 loads in flight, then the adds in list order -- divides, and reduces the averaged row to its arg-max (wave butterfly
//                 with lowest-index tie-break, waves combined in order through LDS)
// No floating-point atomics; two calls on the same input give the same bytes.
#include "internal.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace trexhip {

static constexpr int AVG_THREADS = 256, AVG_MAX_CLASSES = 1024, AVG_MAX_IDS = 65536, AVG_MAX_ROWS = 1 << 24, AVG_UNROLL = 16, AVG_FILL_UNROLL = 8;
static constexpr int AVG_SEG_ROWS = 4096, AVG_MAX_SEGS = 64, AVG_MAX_SLOTS = 1 << 18;   // rows per segment at least, segments and (id, segment) slots at most

struct AvgArgs {
    const float* probs; int n, classes;
    const int32_t* ids; int n_ids;
    int segs, seg_len;               // rows [s * seg_len, min(n, (s + 1) * seg_len)) are segment s
    uint32_t* flag;                  // an id outside 0..n_ids-1
    uint32_t* offs;                  // [n_ids * segs + 1]: counts of (id, segment), id-major, then their exclusive scan; the last entry is the total
    int32_t* list;                   // [n] row indices grouped by id, ascending inside an id
    float* samples;                  // [n_ids]
    float* averages;                 // [n_ids][classes]
    int32_t* max_index;              // [n_ids]
    float* max_p;                    // [n_ids]
};

__global__ __launch_bounds__(AVG_THREADS) void k_avg_count(const AvgArgs A) {
    for (int i = blockIdx.x * AVG_THREADS + threadIdx.x; i < A.n; i += gridDim.x * AVG_THREADS) {
        const int k = A.ids[i];
        if (k < 0 || k >= A.n_ids) atomicOr(A.flag, 1u);
        else atomicAdd(A.offs + (size_t)k * A.segs + i / A.seg_len, 1u);
    }
}

// one workgroup: every thread sums a contiguous piece, the pieces are scanned through LDS, every thread writes its piece's exclusive prefixes
__global__ __launch_bounds__(1024) void k_avg_scan(const AvgArgs A) {
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x, m = A.n_ids * A.segs, per = (m + 1023) / 1024;
    const int a = min(tid * per, m), b = min(a + per, m);
    uint32_t sum = 0;
    for (int i = a; i < b; ++i) sum += A.offs[i];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int t = 0; t < 1024; ++t) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
        A.offs[m] = run;
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (int i = a; i < b; ++i) { const uint32_t v = A.offs[i]; A.offs[i] = run; run += v; }
}

__global__ __launch_bounds__(AVG_THREADS) void k_avg_fill(const AvgArgs A) {
    const int lane = threadIdx.x & 63;
    const int slot = blockIdx.x * (AVG_THREADS / 64) + (threadIdx.x >> 6);          // wave-uniform
    if (slot >= A.n_ids * A.segs || *A.flag) return;
    uint32_t pos = A.offs[slot];
    const uint32_t stop = A.offs[slot + 1];                                         // the (id, segment) holds stop - pos rows
    const int k = slot / A.segs, seg = slot % A.segs;
    const int r_end = min(A.n, (seg + 1) * A.seg_len);
    for (int r0 = seg * A.seg_len; r0 < r_end && pos < stop; r0 += 64 * AVG_FILL_UNROLL) {
        int v[AVG_FILL_UNROLL];
#pragma unroll
        for (int u = 0; u < AVG_FILL_UNROLL; ++u) {
            const int r = r0 + 64 * u + lane;
            v[u] = r < r_end ? A.ids[r] : -1;
        }
#pragma unroll
        for (int u = 0; u < AVG_FILL_UNROLL; ++u) {
            const bool hit = v[u] == k;
            const unsigned long long m = __ballot(hit);
            const uint32_t at = pos + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (hit && at < stop) A.list[at] = r0 + 64 * u + lane;                 // at < stop always, unless d_ids changed under the call
            pos += (uint32_t)__popcll(m);
        }
    }
}

// blockDim.x = 64 * ceil(classes / 64): thread = class
__global__ __launch_bounds__(AVG_MAX_CLASSES) void k_avg_sum(const AvgArgs A) {
    __shared__ uint32_t s_key[AVG_MAX_CLASSES / 64];
    __shared__ int s_arg[AVG_MAX_CLASSES / 64];
    if (*A.flag) return;
    const int k = blockIdx.x, c = threadIdx.x, lane = c & 63, wave = c >> 6, classes = A.classes;
    const bool active = c < classes;
    const uint32_t start = A.offs[(size_t)k * A.segs], end = A.offs[(size_t)(k + 1) * A.segs];
    const float* col = A.probs + (active ? c : 0);                                  // a lane behind the last class reads class 0 and drops it
    float acc = 0.f;
    for (uint32_t base = start; base < end; base += 64) {
        const int m = (int)min(64u, end - base);
        const int mine = lane < m ? A.list[base + lane] : 0;
        int j = 0;
        for (; j + AVG_UNROLL <= m; j += AVG_UNROLL) {
            float v[AVG_UNROLL];
#pragma unroll
            for (int u = 0; u < AVG_UNROLL; ++u) {
                const int r = __shfl(mine, j + u);
                v[u] = col[(size_t)r * classes];
            }
#pragma unroll
            for (int u = 0; u < AVG_UNROLL; ++u) acc += v[u];                       // list order = row order
        }
        for (; j < m; ++j) {
            const int r = __shfl(mine, j);
            acc += col[(size_t)r * classes];
        }
    }
    const uint32_t count = end - start;
    if (count > 0) acc = acc / (float)count;                                         // one correctly rounded division (:177-178); none for an id without rows
    if (active) A.averages[(size_t)k * classes + c] = acc;
    // the scan of check_additional_range (:526-541) on the bit patterns: floats > 0 order like their bits, a NaN is never taken
    const uint32_t bits = __float_as_uint(acc);
    uint32_t best = active && (bits - 1u) < 0x7F800000u ? bits : 0u;
    int arg = best ? c : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ob = __shfl_xor(best, d);
        const int oa = __shfl_xor(arg, d);
        if (ob != 0u && (ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    if (lane == 0) { s_key[wave] = best; s_arg[wave] = arg; }
    __syncthreads();
    if (c != 0) return;
    for (int w = 1; w < (int)blockDim.x / 64; ++w)
        if (s_key[w] > best) { best = s_key[w]; arg = s_arg[w]; }                    // strictly larger: the lower wave = the lower index keeps a tie
    A.samples[k] = (float)count;
    A.max_index[k] = arg;
    A.max_p[k] = __uint_as_float(best);
}

static size_t avg_up16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace trexhip

using namespace trexhip;

extern "C" {

int trexhip_class_averages_device(trexhip_ctx* ctx, const float* d_probs, int32_t n, int32_t classes, const int32_t* d_ids, int32_t n_ids, float* samples,
                                  float* averages, int32_t* max_index, float* max_p) {
    if (!ctx) { set_error("trexhip_class_averages_device: null context"); return TREXHIP_E_INVALID; }
    if (n < 1 || n > AVG_MAX_ROWS) { set_error("trexhip_class_averages_device: n must be 1..2^24 (the sample count is a float)"); return TREXHIP_E_INVALID; }
    if (classes < 1 || classes > AVG_MAX_CLASSES) { set_error("trexhip_class_averages_device: classes must be 1..1024"); return TREXHIP_E_INVALID; }
    if (n_ids < 1 || n_ids > AVG_MAX_IDS) { set_error("trexhip_class_averages_device: n_ids must be 1..65536"); return TREXHIP_E_INVALID; }
    if (!d_probs || !d_ids) { set_error("trexhip_class_averages_device: probabilities and ids are required"); return TREXHIP_E_INVALID; }
    const int segs = std::max(1, std::min({AVG_MAX_SEGS, (n + AVG_SEG_ROWS - 1) / AVG_SEG_ROWS, AVG_MAX_SLOTS / n_ids}));
    const int seg_len = (n + segs - 1) / segs;
    const size_t slots = (size_t)n_ids * segs;
    // one scratch buffer: [flag | max_index | max_p | samples | averages] come back in one copy (as far as they are asked for), the rest stays
    const size_t o_flag = 0, o_maxi = 16, o_maxp = o_maxi + avg_up16((size_t)n_ids * 4), o_samples = o_maxp + avg_up16((size_t)n_ids * 4),
                 o_avg = o_samples + avg_up16((size_t)n_ids * 4), o_offs = o_avg + avg_up16((size_t)n_ids * classes * 4),
                 o_list = o_offs + avg_up16((slots + 1) * 4), total = o_list + avg_up16((size_t)n * 4);
    const size_t back = averages ? o_offs : samples ? o_avg : o_samples;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    if (int rc = ctx->avg.reserve(ctx, total, "trexhip_class_averages_device")) return rc;
    uint8_t* base = ctx->avg.as<uint8_t>();
    TH_CHECK_HIP(hipMemsetAsync(base + o_flag, 0, 16, s));
    TH_CHECK_HIP(hipMemsetAsync(base + o_offs, 0, (slots + 1) * 4, s));
    AvgArgs A{};
    A.probs = d_probs; A.n = n; A.classes = classes;
    A.ids = d_ids; A.n_ids = n_ids;
    A.segs = segs; A.seg_len = seg_len;
    A.flag = reinterpret_cast<uint32_t*>(base + o_flag);
    A.offs = reinterpret_cast<uint32_t*>(base + o_offs);
    A.list = reinterpret_cast<int32_t*>(base + o_list);
    A.samples = reinterpret_cast<float*>(base + o_samples);
    A.averages = reinterpret_cast<float*>(base + o_avg);
    A.max_index = reinterpret_cast<int32_t*>(base + o_maxi);
    A.max_p = reinterpret_cast<float*>(base + o_maxp);
    const int waves_per_block = AVG_THREADS / 64;
    hipLaunchKernelGGL(k_avg_count, dim3(std::min(2048, (n + AVG_THREADS - 1) / AVG_THREADS)), dim3(AVG_THREADS), 0, s, A);
    hipLaunchKernelGGL(k_avg_scan, dim3(1), dim3(1024), 0, s, A);
    hipLaunchKernelGGL(k_avg_fill, dim3((unsigned)((slots + waves_per_block - 1) / waves_per_block)), dim3(AVG_THREADS), 0, s, A);
    hipLaunchKernelGGL(k_avg_sum, dim3(n_ids), dim3((classes + 63) / 64 * 64), 0, s, A);
    TH_CHECK_HIP(hipGetLastError());
    std::vector<uint8_t> host(back);
    TH_CHECK_HIP(hipMemcpyAsync(host.data(), base, back, hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    uint32_t flag;
    std::memcpy(&flag, host.data() + o_flag, 4);
    if (flag) { set_error("trexhip_class_averages_device: an id was outside 0..n_ids-1; no output was written"); return TREXHIP_E_INVALID; }
    if (max_index) std::memcpy(max_index, host.data() + o_maxi, (size_t)n_ids * 4);
    if (max_p) std::memcpy(max_p, host.data() + o_maxp, (size_t)n_ids * 4);
    if (samples) std::memcpy(samples, host.data() + o_samples, (size_t)n_ids * 4);
    if (averages) std::memcpy(averages, host.data() + o_avg, (size_t)n_ids * classes * 4);
    return TREXHIP_OK;
}

}  // extern "C"
