// validate.hip -- the two reductions of the end-of-epoch validation of identity training, on probabilities that are already in HBM.
//
// Replaces, for softmax rows [n][classes] (trexhip_train_predict_device's or trexhip_identify_device's):
//   Accumulation::calculate_uniqueness, Application/src/tracker/ui/Accumulation.cpp:799-878 -- per frame (a range of rows) the set of
//       distinct arg-max identities and the largest probability each got -> unique_percent_raw / unique_percent, good / bad frames,
//       the means over the frames and the per-identity means (:865-870)
//   the counting of ValidationCallback.plot_comparison_raw, visual_recognition_torch.py:406-451, column 3 -- (y.argmax(axis=1) == i).sum() / len(y)
//       per class = the diagonal of the confusion matrix over its row sums
// One launch (k_val_reduce: workgroups 0 .. n_frames-1 take one frame each, the workgroups behind them 64 rows of the confusion matrix each)
// plus a finalise (k_val_finalize: the sums over the frames, in frame order), then one copy to the host.
//
// The two arg-maxes differ, as they do in the reference:
//   identity of a row (:804-814): max_p = 0, ids ascending, take id iff p > max_p -- the first index of the largest entry that is > 0; a row
//       without one (all zero, all negative, NaN only) has NO identity and adds nothing to its frame
//   confusion column: np.argmax -- the first NaN if the row holds one, else the first index of the largest entry (-0 == +0)
// Both are taken on the bit patterns (non-negative floats order like their bits), so a denormal maximum counts in any float mode.
//
// Order of every floating-point sum is fixed, so two runs give the same bytes: accum_p (:826-832) over a frame's identities in ASCENDING
// identity order (the reference iterates a hash_map: its order is unspecified), float32; percentages / rpercentages (:841, :850) in double in
// frame order; unique_percent_per_identity (:830) in float32 in frame order.  The confusion matrix is integer atomics.
#include "internal.h"
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace trexhip {

static constexpr int VAL_THREADS = 256, VAL_WAVES = VAL_THREADS / 64, VAL_CONF_ROWS = 64, VAL_MAX_CLASSES = 1024;

// key of an entry for the identity arg-max: its bits if it is > 0 (not NaN), else 0
__device__ __forceinline__ uint32_t key_identity(uint32_t b) { return (b - 1u) < 0x7F800000u ? b : 0u; }
// key for np.argmax: NaN above everything, -0 == +0, else the usual order-preserving map of the bits
__device__ __forceinline__ uint32_t key_argmax(uint32_t b) {
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one wave, one row: (largest key, first index that has it).  Lanes walk the classes ascending and keep their first maximum; the butterfly
// prefers the lower index among equal keys
template <bool IDENTITY>
__device__ __forceinline__ void row_argmax(const float* __restrict__ row, const int classes, const bool vec4, const int lane, uint32_t& best, int& arg) {
    best = 0u;
    arg = IDENTITY ? -1 : 0x7FFFFFFF;
    auto take = [&](const float v, const int c) {
        const uint32_t b = __float_as_uint(v);
        const uint32_t k = IDENTITY ? key_identity(b) : key_argmax(b);
        if (IDENTITY ? (k > best) : (k > best || arg == 0x7FFFFFFF)) { best = k; arg = c; }
    };
    if (vec4) {
        const float4* r4 = reinterpret_cast<const float4*>(row);
        for (int q = lane; q < classes / 4; q += 64) {
            const float4 v = r4[q];
            take(v.x, 4 * q); take(v.y, 4 * q + 1); take(v.z, 4 * q + 2); take(v.w, 4 * q + 3);
        }
    } else {
        for (int c = lane; c < classes; c += 64) take(row[c], c);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ob = __shfl_xor(best, d);
        const int oa = __shfl_xor(arg, d);
        const bool mine_valid = IDENTITY ? best != 0u : arg != 0x7FFFFFFF, other_valid = IDENTITY ? ob != 0u : oa != 0x7FFFFFFF;
        if (other_valid && (!mine_valid || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
}

struct ValArgs {
    const float* probs; int n, classes, vec4;
    const int32_t* targets;          // [n] or null
    const int32_t* ranges;           // [n_frames][2] or null
    int n_frames;
    float normal;                    // 1 + expf(-float(M_PI))   (:835)
    uint32_t* confusion;             // [classes][classes], zeroed by the caller
    uint32_t* flag;                  // a target outside 0..classes-1
    float *up, *upr;                 // [n_frames] unique_percent, unique_percent_raw
    double *pd, *rpd;                // [n_frames] the same as the doubles the reference sums
    uint32_t* good;                  // [n_frames]
    float* cls_tab;                  // [n_frames][classes] largest max_p of the identity in the frame, 0 = not seen; or null
    float* per_class;                // [classes]
    float* result;                   // trexhip_uniqueness_result
};

__global__ __launch_bounds__(VAL_THREADS) void k_val_reduce(const ValArgs A) {
    __shared__ uint32_t s_max[VAL_MAX_CLASSES];          // bits of the largest max_p per identity (0 = none: a max_p is > 0)
    __shared__ uint32_t s_bits[VAL_MAX_CLASSES / 32];    // presence bitmap
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, classes = A.classes;
    if ((int)blockIdx.x >= A.n_frames) {
        // ---- confusion[target][np.argmax(row)] += 1
        const int r0 = ((int)blockIdx.x - A.n_frames) * VAL_CONF_ROWS;
        const int r1 = min(r0 + VAL_CONF_ROWS, A.n);
        for (int r = r0 + wave; r < r1; r += VAL_WAVES) {
            uint32_t best; int arg;
            row_argmax<false>(A.probs + (size_t)r * classes, classes, A.vec4 != 0, lane, best, arg);
            if (lane == 0) {
                const int t = A.targets[r];
                if (t < 0 || t >= classes) atomicOr(A.flag, 1u);
                else atomicAdd(A.confusion + (size_t)t * classes + arg, 1u);
            }
        }
        return;
    }
    // ---- one frame
    const int f = blockIdx.x, start = A.ranges[2 * f], end = A.ranges[2 * f + 1], length = end - start;   // 0 <= start <= end <= n (checked by the host)
    for (int c = tid; c < classes; c += VAL_THREADS) s_max[c] = 0u;
    if (tid < VAL_MAX_CLASSES / 32) s_bits[tid] = 0u;
    __syncthreads();
    for (int r = start + wave; r < end; r += VAL_WAVES) {
        uint32_t best; int arg;
        row_argmax<true>(A.probs + (size_t)r * classes, classes, A.vec4 != 0, lane, best, arg);
        if (lane == 0 && best != 0u) {
            atomicMax(&s_max[arg], best);                 // probs[max_id] = max(probs[max_id], max_p)   (:818)
            atomicOr(&s_bits[arg >> 5], 1u << (arg & 31));
        }
    }
    __syncthreads();
    if (A.cls_tab)
        for (int c = tid; c < classes; c += VAL_THREADS) A.cls_tab[(size_t)f * classes + c] = __uint_as_float(s_max[c]);
    if (tid != 0) return;
    int distinct = 0;
    float accum_p = 0.f;
    for (int w = 0; w < (classes + 31) / 32; ++w) {       // ascending identity order
        uint32_t m = s_bits[w];
        distinct += __popc(m);
        while (m) {
            const int b = __ffs(m) - 1;
            m &= m - 1u;
            accum_p += __uint_as_float(s_max[32 * w + b]);
        }
    }
    const float rawf = length <= 0 ? 0.f : (float)distinct / (float)length;      // unique_ids.size() / float(range.length())   (:822-824)
    double p = (double)rawf;
    const double rp = p;
    if (distinct > 0) {
        const float x = accum_p / (float)distinct;
        const double e = exp(-(double)x * 3.14159265358979323846);
        p = 1.0 / (1.0 + e) * (double)A.normal * p;        // logic_regression(accum_p / float(probs.size())) * p   (:834-845)
    }
    A.upr[f] = rawf;
    A.up[f] = (float)p;
    A.pd[f] = p;
    A.rpd[f] = rp;
    A.good[f] = distinct == length ? 1u : 0u;             // (:852)
}

// the sums over the frames, in frame order: thread 0 the three scalars, one thread per identity its mean
__global__ __launch_bounds__(VAL_THREADS) void k_val_finalize(const ValArgs A) {
    const int tid = threadIdx.x;
    if (A.cls_tab)
        for (int c = tid; c < A.classes; c += VAL_THREADS) {
            float sum = 0.f, count = 0.f;                  // unique_percent_per_identity[id] += p; ++per_identity_samples[id]   (:830-831)
            for (int f = 0; f < A.n_frames; ++f) {
                const float v = A.cls_tab[(size_t)f * A.classes + c];
                if (__float_as_uint(v) != 0u) { sum += v; count += 1.f; }
            }
            A.per_class[c] = count > 0.f ? sum / count : 0.f;
        }
    if (tid != 0) return;
    double percentages = 0.0, rpercentages = 0.0;
    uint32_t good = 0;
    for (int f = 0; f < A.n_frames; ++f) { percentages += A.pd[f]; rpercentages += A.rpd[f]; good += A.good[f]; }
    const uint32_t bad = (uint32_t)A.n_frames - good;
    reinterpret_cast<uint32_t*>(A.result)[0] = good;
    reinterpret_cast<uint32_t*>(A.result)[1] = bad;
    A.result[2] = (float)good / (float)(good + bad);
    A.result[3] = (float)(percentages / (double)A.n_frames);
    A.result[4] = (float)(rpercentages / (double)A.n_frames);
}

static size_t up16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace trexhip

using namespace trexhip;

extern "C" {

int trexhip_validation_metrics_device(trexhip_ctx* ctx, const float* d_probs, int32_t n, int32_t classes, const int32_t* d_targets,
                                      const int32_t* frame_ranges, int32_t n_frames, uint32_t* confusion, trexhip_uniqueness_result* result,
                                      float* unique_percent, float* unique_percent_raw, float* uniqueness_per_class) {
    static_assert(sizeof(trexhip_uniqueness_result) == 20, "trexhip_uniqueness_result is five 32-bit words");
    if (!ctx) { set_error("trexhip_validation_metrics_device: null context"); return TREXHIP_E_INVALID; }
    if (classes < 1 || classes > VAL_MAX_CLASSES) { set_error("trexhip_validation_metrics_device: classes must be 1..1024"); return TREXHIP_E_INVALID; }
    if (n < 0 || (n > 0 && !d_probs)) { set_error("trexhip_validation_metrics_device: n >= 0 rows of probabilities are required"); return TREXHIP_E_INVALID; }
    if (d_targets && !confusion) { set_error("trexhip_validation_metrics_device: targets without a confusion matrix to fill"); return TREXHIP_E_INVALID; }
    const bool frames = frame_ranges != nullptr, conf = d_targets != nullptr;
    if (frames) {
        if (n_frames < 1) { set_error("trexhip_validation_metrics_device: frame ranges given, n_frames must be at least 1"); return TREXHIP_E_INVALID; }
        for (int f = 0; f < n_frames; ++f) {
            const int32_t a = frame_ranges[2 * f], b = frame_ranges[2 * f + 1];
            if (a < 0 || a > b || b > n) {
                set_error("trexhip_validation_metrics_device: frame_ranges[" + std::to_string(f) + "] = {" + std::to_string(a) + ", " + std::to_string(b) +
                          "} must satisfy 0 <= start <= end <= n = " + std::to_string(n));
                return TREXHIP_E_INVALID;
            }
        }
    }
    const int nf = frames ? n_frames : 0;
    const bool per_class = frames && uniqueness_per_class != nullptr;
    // one scratch buffer: [flag | result | unique_percent | unique_percent_raw | per-class means | confusion] come back in one copy, the rest stays
    const size_t o_flag = 0, o_result = 16, o_up = 48, o_upr = o_up + up16((size_t)nf * 4), o_pc = o_upr + up16((size_t)nf * 4),
                 o_conf = o_pc + up16(per_class ? (size_t)classes * 4 : 0), o_back = o_conf + up16(conf ? (size_t)classes * classes * 4 : 0),
                 o_ranges = o_back, o_pd = o_ranges + up16((size_t)nf * 8), o_rpd = o_pd + up16((size_t)nf * 8), o_good = o_rpd + up16((size_t)nf * 8),
                 o_tab = o_good + up16((size_t)nf * 4), total = o_tab + up16(per_class ? (size_t)nf * classes * 4 : 0);
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    if (int rc = ctx->val.reserve(ctx, total, "trexhip_validation_metrics_device")) return rc;
    uint8_t* base = ctx->val.as<uint8_t>();
    TH_CHECK_HIP(hipMemsetAsync(base, 0, o_conf + (conf ? (size_t)classes * classes * 4 : 0), s));   // flag, outputs and the confusion counts
    if (frames) TH_CHECK_HIP(hipMemcpyAsync(base + o_ranges, frame_ranges, (size_t)nf * 8, hipMemcpyHostToDevice, s));   // pageable source: staged before the call returns
    ValArgs A{};
    A.probs = d_probs; A.n = n; A.classes = classes;
    A.vec4 = (classes % 4 == 0 && reinterpret_cast<uintptr_t>(d_probs) % 16 == 0) ? 1 : 0;
    A.targets = d_targets;
    A.ranges = reinterpret_cast<const int32_t*>(base + o_ranges);
    A.n_frames = nf;
    A.normal = 1.0f + expf(-1.0f * (float)M_PI * 1.0f);
    A.confusion = reinterpret_cast<uint32_t*>(base + o_conf);
    A.flag = reinterpret_cast<uint32_t*>(base + o_flag);
    A.up = reinterpret_cast<float*>(base + o_up); A.upr = reinterpret_cast<float*>(base + o_upr);
    A.pd = reinterpret_cast<double*>(base + o_pd); A.rpd = reinterpret_cast<double*>(base + o_rpd);
    A.good = reinterpret_cast<uint32_t*>(base + o_good);
    A.cls_tab = per_class ? reinterpret_cast<float*>(base + o_tab) : nullptr;
    A.per_class = reinterpret_cast<float*>(base + o_pc);
    A.result = reinterpret_cast<float*>(base + o_result);
    const int conf_blocks = conf ? (n + VAL_CONF_ROWS - 1) / VAL_CONF_ROWS : 0;
    if (nf + conf_blocks > 0) hipLaunchKernelGGL(k_val_reduce, dim3(nf + conf_blocks), dim3(VAL_THREADS), 0, s, A);
    if (frames) hipLaunchKernelGGL(k_val_finalize, dim3(1), dim3(VAL_THREADS), 0, s, A);
    TH_CHECK_HIP(hipGetLastError());
    std::vector<uint8_t> host(o_back);
    TH_CHECK_HIP(hipMemcpyAsync(host.data(), base, o_back, hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    uint32_t flag;
    std::memcpy(&flag, host.data() + o_flag, 4);
    if (flag) { set_error("trexhip_validation_metrics_device: a target class index was outside 0..classes-1; no output was written"); return TREXHIP_E_INVALID; }
    if (conf) std::memcpy(confusion, host.data() + o_conf, (size_t)classes * classes * 4);
    if (frames) {
        if (result) std::memcpy(result, host.data() + o_result, sizeof(*result));
        if (unique_percent) std::memcpy(unique_percent, host.data() + o_up, (size_t)nf * 4);
        if (unique_percent_raw) std::memcpy(unique_percent_raw, host.data() + o_upr, (size_t)nf * 4);
        if (per_class) std::memcpy(uniqueness_per_class, host.data() + o_pc, (size_t)classes * 4);
    }
    return TREXHIP_OK;
}

}  // extern "C"
