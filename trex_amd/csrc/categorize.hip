// categorize.hip -- categorisation on the device: the entry points of the category network (its chain: cnn_arch.hip) and the tracklet vote.
//
// Replaces, for crops that are already in HBM:
//   ui/Categorize.cpp:730-761             py::set_variable("images", ..) + py::run(module, "predict") + receive(std::vector<float>): one label per image
//   CategorizeDatastore.cpp:555-585,      DataStore::label_averaged / the counting of a sample's labels: per tracklet the number of rows per category,
//   CategorizeInterface.cpp:212-247       the first maximum, and counts / float(rows)
//
//   k_vote_check          a tracklet id outside [0, T) raises a flag word; the host reads it BEFORE anything is written (the checked pass)
//   k_tracklet_vote       counts[T][C] and rows[T] by integer adds only, so the result does not depend on the order of the rows.  Where the whole table
//                         fits a workgroup's LDS -- T * (C + 1) <= VOTE_LDS_WORDS = 4096 words, 16 KB -- every workgroup counts its rows in LDS and
//                         adds the non-zero words to HBM once (the contended case: all rows in one tracklet is one LDS word per label, not one HBM
//                         word for the whole grid); larger tables take one global atomic add per row and one for its tracklet's row count.
//                         Reads 8 bytes per row; bounded by the atomics: LDS atomics below the switch, L2 atomics above it
//   k_vote_final          one thread per tracklet: the first maximum of its counts (std::max_element), -1 when that maximum is 0, and
//                         share[c] = __fdiv_rn((float)counts[c], (float)rows) (0 for an empty tracklet).  Reads the table once
#include "cnn_arch.h"
#include "cnn_weights.h"
#include <cstring>

namespace trexhip {
namespace {

constexpr int VOTE_LDS_WORDS = 4096;
constexpr int VOTE_THREADS = 256;

__global__ __launch_bounds__(VOTE_THREADS) void k_vote_check(const int32_t* __restrict__ tracklet, const int n, const int T, uint32_t* __restrict__ flag) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * VOTE_THREADS + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * VOTE_THREADS) {
        const int32_t t = tracklet[i];
        bad |= t < 0 || t >= T;
    }
    if (bad) atomicOr(flag, 1u);
}

// words[0 .. T*C) = counts, words[T*C .. T*C + T) = rows (the caller lays counts and rows out apart in HBM; in LDS they are one array)
template <bool LDS>
__global__ __launch_bounds__(VOTE_THREADS) void k_tracklet_vote(const int32_t* __restrict__ labels, const int32_t* __restrict__ tracklet, const int n, const int T,
                                                                const int C, uint32_t* __restrict__ counts, uint32_t* __restrict__ rows,
                                                                uint32_t* __restrict__ skipped) {
    __shared__ uint32_t hist[LDS ? VOTE_LDS_WORDS : 1];
    const int words = T * (C + 1);
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < words; i += VOTE_THREADS) hist[i] = 0u;
        __syncthreads();
    }
    uint32_t skip = 0;
    for (size_t i = (size_t)blockIdx.x * VOTE_THREADS + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * VOTE_THREADS) {
        const int32_t t = tracklet[i], l = labels[i];                  // t is in range: k_vote_check ran first
        if constexpr (LDS) atomicAdd(&hist[T * C + t], 1u); else atomicAdd(&rows[t], 1u);      // every row handed in counts as a row
        if (l < 0) continue;                                           // no label
        if (l >= C) { ++skip; continue; }                              // the reference warns and goes on
        if constexpr (LDS) atomicAdd(&hist[t * C + l], 1u); else atomicAdd(&counts[(size_t)t * C + l], 1u);
    }
    if (skip) atomicAdd(skipped, skip);
    if constexpr (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += VOTE_THREADS) {
            const uint32_t v = hist[i];
            if (v) atomicAdd(i < T * C ? &counts[i] : &rows[i - T * C], v);
        }
    }
}

__global__ __launch_bounds__(VOTE_THREADS) void k_vote_final(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ rows, const int T, const int C,
                                                             int32_t* __restrict__ label, float* __restrict__ share) {
    const int t = blockIdx.x * VOTE_THREADS + threadIdx.x;
    if (t >= T) return;
    const uint32_t* c = counts + (size_t)t * C;
    const uint32_t r = rows[t];
    uint32_t best = 0;
    int at = 0;
    for (int k = 0; k < C; ++k) {
        const uint32_t v = c[k];
        if (v > best) { best = v; at = k; }                            // strictly larger: the first maximum stays
        if (share) share[(size_t)t * C + k] = r ? __fdiv_rn((float)v, (float)r) : 0.f;
    }
    label[t] = best ? at : -1;
}

int category_prepare(trexhip_ctx* ctx, const bool args, const char* who, const int32_t n, Net** net) {
    *net = nullptr;
    if (!args) { set_error(std::string(who) + ": null argument"); return TREXHIP_E_INVALID; }
    Net* loaded = static_cast<Net*>(ctx->cat);
    if (!loaded) { set_error(std::string(who) + ": no category weights loaded (trexhip_categorize_load_weights)"); return TREXHIP_E_INVALID; }
    if (n < 0) { set_error(std::string(who) + ": n < 0"); return TREXHIP_E_INVALID; }
    if (n == 0) return TREXHIP_OK;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    const int rc = arch_ensure_act(ctx, loaded, n, who);
    if (rc == TREXHIP_OK) *net = loaded;
    return rc;
}

// the guard words of the category network are its own (Net::d_ovf of ctx->cat): the identity network's statistics never see a category call
int category_forward(trexhip_ctx* ctx, Net* net, const uint8_t* d_crops, const int n, int32_t* d_labels, float* d_probs, float* d_logits) {
    const bool h16 = ctx->cnn_mode == TREXHIP_CNN_FP16X3;
    if (h16) {
        if (!net->ovf_clean) TH_CHECK_HIP(hipMemsetAsync(net->d_ovf, 0, OVF_PLAN * 4, ctx->stream));
        net->ovf_clean = false;
    }
    const int rc = arch_forward(ctx, *net, d_crops, n, d_probs ? d_probs : net->probs, d_logits ? d_logits : net->logits, d_labels);
    if (rc == TREXHIP_OK) { net->last_mode = ctx->cnn_mode; if (h16) net->ovf_clean = true; }
    return rc;
}

}  // namespace
}  // namespace trexhip

using namespace trexhip;

extern "C" {

int trexhip_categorize_load_weights(trexhip_ctx* ctx, const void* blob, size_t bytes) {
    if (!ctx || !blob) { set_error("trexhip_categorize_load_weights: null argument"); return TREXHIP_E_INVALID; }
    return category_load(ctx, blob, bytes);
}

int trexhip_categorize_info(trexhip_ctx* ctx, int32_t* categories, int32_t* channels, int32_t* width, int32_t* height) {
    if (!ctx) { set_error("trexhip_categorize_info: null context"); return TREXHIP_E_INVALID; }
    const Net* net = static_cast<const Net*>(ctx->cat);
    if (categories) *categories = net ? net->classes : 0;
    if (channels) *channels = net ? net->CH : 0;
    if (width) *width = net ? net->W : 0;
    if (height) *height = net ? net->H : 0;
    return TREXHIP_OK;
}

size_t trexhip_categorize_blob_bytes(int32_t categories, int32_t channels, int32_t width, int32_t height) {
    return category_blob_bytes(categories, channels, width, height);
}

int trexhip_categorize_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n, int32_t* d_labels, float* d_probs, float* d_logits) {
    Net* net;
    const int rc = category_prepare(ctx, ctx && d_crops && d_labels, "trexhip_categorize_device", n, &net);
    if (rc || !net) return rc;
    return category_forward(ctx, net, d_crops, n, d_labels, d_probs, d_logits);
}

int trexhip_categorize(trexhip_ctx* ctx, const uint8_t* crops, int32_t n, int32_t* labels) {
    Net* net;
    int rc = category_prepare(ctx, ctx && crops && labels, "trexhip_categorize", n, &net);
    if (rc || !net) return rc;
    ArchNet& a = *net->arch;
    TH_CHECK_HIP(hipMemcpyAsync(net->crops, crops, (size_t)net->W * net->H * net->CH * n, hipMemcpyHostToDevice, ctx->stream));
    rc = category_forward(ctx, net, net->crops, n, a.labels, nullptr, nullptr);
    if (rc) return rc;
    TH_CHECK_HIP(hipMemcpyAsync(a.h_labels, a.labels, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(labels, a.h_labels, (size_t)n * 4);
    return TREXHIP_OK;
}

int trexhip_tracklet_labels_device(trexhip_ctx* ctx, const int32_t* d_labels, const int32_t* d_tracklet, int32_t n, int32_t n_tracklets, int32_t categories,
                                   uint32_t* d_counts, uint32_t* d_rows, int32_t* d_label, float* d_share, uint32_t* skipped) {
    const char* who = "trexhip_tracklet_labels_device";
    if (!ctx) { set_error(std::string(who) + ": null context"); return TREXHIP_E_INVALID; }
    if (n < 0) { set_error(std::string(who) + ": n < 0"); return TREXHIP_E_INVALID; }
    if (n == 0) { if (skipped) *skipped = 0; return TREXHIP_OK; }
    if (!d_labels || !d_tracklet || !d_counts || !d_rows || !d_label) { set_error(std::string(who) + ": null argument"); return TREXHIP_E_INVALID; }
    if (n_tracklets < 1 || n_tracklets > (1 << 24)) { set_error(std::string(who) + ": n_tracklets must be 1..2^24"); return TREXHIP_E_INVALID; }
    if (categories < 1 || categories > 1024) { set_error(std::string(who) + ": categories must be 1..1024"); return TREXHIP_E_INVALID; }
    const int T = n_tracklets, C = categories;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    if (int rc = ctx->vote.reserve(ctx, 16, who)) return rc;
    uint32_t* w = ctx->vote.as<uint32_t>();                            // [0] flag, [1] skipped
    TH_CHECK_HIP(hipMemsetAsync(w, 0, 16, s));
    const int grid = std::max(1, std::min(4 * ctx->n_cus, (n + VOTE_THREADS - 1) / VOTE_THREADS));
    hipLaunchKernelGGL(k_vote_check, dim3(grid), dim3(VOTE_THREADS), 0, s, d_tracklet, n, T, w);
    uint32_t host[2] = {0, 0};
    TH_CHECK_HIP(hipMemcpyAsync(host, w, 4, hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    if (host[0]) { set_error(std::string(who) + ": a tracklet id was outside 0..n_tracklets-1; no output was written"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipMemsetAsync(d_counts, 0, (size_t)T * C * 4, s));
    TH_CHECK_HIP(hipMemsetAsync(d_rows, 0, (size_t)T * 4, s));
    if ((size_t)T * (C + 1) <= (size_t)VOTE_LDS_WORDS)
        hipLaunchKernelGGL(k_tracklet_vote<true>, dim3(grid), dim3(VOTE_THREADS), 0, s, d_labels, d_tracklet, n, T, C, d_counts, d_rows, w + 1);
    else
        hipLaunchKernelGGL(k_tracklet_vote<false>, dim3(grid), dim3(VOTE_THREADS), 0, s, d_labels, d_tracklet, n, T, C, d_counts, d_rows, w + 1);
    hipLaunchKernelGGL(k_vote_final, dim3((T + VOTE_THREADS - 1) / VOTE_THREADS), dim3(VOTE_THREADS), 0, s, d_counts, d_rows, T, C, d_label, d_share);
    TH_CHECK_HIP(hipGetLastError());
    TH_CHECK_HIP(hipMemcpyAsync(host, w, 8, hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    if (skipped) *skipped = host[1];
    return TREXHIP_OK;
}

}  // extern "C"
