// capi.hip -- C ABI of libtrexhip (include/trexhip.h): context, memory, background, segment, fetch.
#include "internal.h"
#include "cnn_plan.h"
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <new>
#include <vector>

namespace trexhip {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }

static void stage_fold(Stage& s, bool all) {
    // fold finished intervals into the totals; `all` waits for the outstanding ones too
    size_t keep = 0;
    for (size_t i = 0; i < s.pending.size(); ++i) {
        EvPair p = s.pending[i];
        hipError_t q = all ? hipEventSynchronize(p.b) : hipEventQuery(p.b);
        float ms = 0.f;
        if (q == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            s.total_ms += ms; s.launches++;
            s.freelist.push_back(p);
        } else if (q == hipErrorNotReady) {
            s.pending[keep++] = p;
        } else {
            (void)hipGetLastError();
            s.freelist.push_back(p);
        }
    }
    s.pending.resize(keep);
}
void stage_begin(trexhip_ctx* ctx, int stage) {
    if (!ctx->profiling) return;
    Stage& s = ctx->stages[stage];
    if (s.pending.size() > 1024) stage_fold(s, false);
    EvPair p;
    if (!s.freelist.empty()) { p = s.freelist.back(); s.freelist.pop_back(); }
    else {
        // timing events only: no system-scope fence when one is recorded (hipEventDisableSystemFence -- "can be used for events that are only being used
        // to measure timing ... avoiding the cost of cache writeback and invalidation, and the performance impact of those actions on the execution of
        // following work", hip_runtime_api.h).  A default event between the pixel pass and the labelling kernel wrote back and invalidated the L2 the
        // labelling kernel was about to read (round 6: the detect pass read 280 us through its own timers and 270 us on the wall clock without them)
        hipEventCreateWithFlags(&p.a, hipEventDisableSystemFence); hipEventCreateWithFlags(&p.b, hipEventDisableSystemFence);
    }
    hipEventRecord(p.a, ctx->stream);
    s.cur = p;
}
void stage_end(trexhip_ctx* ctx, int stage) {
    if (!ctx->profiling) return;
    Stage& s = ctx->stages[stage];
    if (!s.cur.a) return;
    hipEventRecord(s.cur.b, ctx->stream);
    s.pending.push_back(s.cur);
    s.cur = EvPair();
}
void stage_read(trexhip_ctx* ctx, int stage) { stage_fold(ctx->stages[stage], true); }
void stage_free(trexhip_ctx* ctx) {
    for (auto& s : ctx->stages) {
        stage_fold(s, true);
        for (auto& p : s.freelist) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
        s.freelist.clear();
    }
}

// one table set (pooled outputs, pinned mirrors, labelling state) from the context's capacities; d_totals is allocated unless the caller has set it
static int alloc_tables(Mem& m, BlobTables& t, LabelState& l, size_t B, size_t H, size_t R, size_t NB, size_t P, size_t pix_ch, const char* who) {
    int rc = TREXHIP_OK;
#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)
    TRY(m.device(&l.d_row_cnt, B * H, who)); TRY(m.device(&l.d_row_base, B * (H + 1), who)); TRY(m.device(&l.d_raster, B * R, who));
    TRY(m.device(&l.d_parent, B * R, who)); TRY(m.device(&l.d_root_ord, B * R, who)); TRY(m.device(&l.d_cnt_runs, B * R, who));
    TRY(m.device(&l.d_cnt_px, B * R, who)); TRY(m.device(&l.d_cur_run, B * R, who)); TRY(m.device(&l.d_pix_begin, B * R, who));
    TRY(m.device(&l.d_blob_map, B * R, who));
    if (!t.d_totals) TRY(m.device(&t.d_totals, 4, who));
    TRY(m.device(&t.d_info, B, who)); TRY(m.device(&t.d_blobs, B * NB, who)); TRY(m.device(&t.d_blob_frame, B * NB, who));
    TRY(m.device(&t.d_runs, B * R, who)); TRY(m.device(&t.d_pixels, B * P * pix_ch, who));
    TRY(m.pinned(&t.h_info, B, who)); TRY(m.pinned(&t.h_totals, 4, who)); TRY(m.pinned(&t.h_blobs, B * NB, who));
    TRY(m.pinned(&t.h_runs, B * R, who)); TRY(m.pinned(&t.h_pixels, B * P * pix_ch, who));
#undef TRY
    return rc;
}

// frame table and totals of the set's batch into the pinned mirrors, then wait for them
static int fetch_info(trexhip_ctx* ctx, BlobTables& t) {
    TH_CHECK_HIP(hipMemcpyAsync(t.h_info, t.d_info, sizeof(trexhip_frame_info) * t.valid_n, hipMemcpyDeviceToHost, ctx->stream));
    TH_CHECK_HIP(hipMemcpyAsync(t.h_totals, t.d_totals, sizeof(uint32_t) * 4, hipMemcpyDeviceToHost, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return TREXHIP_OK;
}

// the rest of a fetch, once h_info and h_totals are in: clamp the totals to the pools (frames that overflowed the pool reserved nothing valid),
// copy the filled parts of the three tables unless a kernel has already exported them, wait -- or (begin) record the context's event behind the
// copies and leave the wait to fetch_wait --, and fill the caller's result
int fetch_wait(trexhip_ctx* ctx) {
    if (!ctx->fetch_pending) return TREXHIP_OK;
    ctx->fetch_pending = false;
    TH_CHECK_HIP(hipEventSynchronize(ctx->fetch_ev));
    return TREXHIP_OK;
}
static int fetch_tables(trexhip_ctx* ctx, BlobTables& t, bool copy, trexhip_batch_result* out, bool begin = false) {
    std::memset(out, 0, sizeof(*out));
    out->n_frames = t.valid_n;
    out->frames = t.h_info; out->blobs = t.h_blobs; out->runs = t.h_runs; out->pixels = t.h_pixels;
    out->pixel_channels = (uint32_t)ctx->pix_ch;
    if (t.valid_n == 0) return TREXHIP_OK;
    const uint32_t tb = std::min(t.h_totals[0], ctx->cfg.pool_blobs), tr = std::min(t.h_totals[1], ctx->cfg.pool_runs), tp = std::min(t.h_totals[2], ctx->cfg.pool_pixels);
    if (copy) {
        hipStream_t s = ctx->stream;
        if (tb) TH_CHECK_HIP(hipMemcpyAsync(t.h_blobs, t.d_blobs, sizeof(trexhip_blob) * tb, hipMemcpyDeviceToHost, s));
        if (tr) TH_CHECK_HIP(hipMemcpyAsync(t.h_runs, t.d_runs, sizeof(trexhip_run) * tr, hipMemcpyDeviceToHost, s));
        if (tp) TH_CHECK_HIP(hipMemcpyAsync(t.h_pixels, t.d_pixels, (size_t)tp * ctx->pix_ch, hipMemcpyDeviceToHost, s));
        if (begin) {
            if (!ctx->fetch_ev) TH_CHECK_HIP(hipEventCreateWithFlags(&ctx->fetch_ev, hipEventDisableTiming));
            TH_CHECK_HIP(hipEventRecord(ctx->fetch_ev, s));
            ctx->fetch_stream = s;
            ctx->fetch_pending = true;
        }
        else TH_CHECK_HIP(hipStreamSynchronize(s));
    }
    out->total_blobs = tb; out->total_runs = tr; out->total_pixels = tp;
    t.fetched = true;
    return TREXHIP_OK;
}

static int fill_cfg(trexhip_ctx* ctx) {
    const trexhip_params& p = ctx->p;
    SegCfg& c = ctx->cfg;
    c.W = p.width; c.H = p.height; c.B = p.max_batch; c.ctr_frames = p.max_batch; c.R = p.max_runs;
    c.T = p.height * TREXHIP_ROW_SLOT + p.max_runs;
    const int thr = p.threshold < 0 ? -p.threshold : p.threshold;   // abs(threshold), as the reference does
    if (p.threshold_maximum < 255) { c.tmin = thr; c.tmax = p.threshold_maximum; }   // cv::inRange
    else { c.tmin = p.inclusive ? thr : thr + 1; c.tmax = 255; }                      // inclusive (default): |p| < threshold is disregarded; 0: strict, cv::threshold
    c.enable_diff = p.enable_difference; c.absdiff = p.absolute_difference;
    c.invert = p.image_invert; c.zero_bg = p.zero_is_background;
    c.slack = p.connectivity == 4 ? 0 : 1;
    c.n_ranges = p.n_ranges;
    c.sqcm = (float)(p.cm_per_pixel * p.cm_per_pixel);
    for (int i = 0; i < 16; ++i) c.ranges[i] = p.ranges[i];
    c.pool_blobs = (uint32_t)p.max_batch * (uint32_t)p.max_blobs;
    c.pool_runs = (uint32_t)p.max_batch * (uint32_t)p.max_runs;
    c.pool_pixels = (uint32_t)p.max_batch * (uint32_t)p.max_pixels;
    c.cap_blobs = (uint32_t)p.max_blobs; c.cap_pixels = (uint32_t)p.max_pixels;
    return TREXHIP_OK;
}

}  // namespace trexhip

using namespace trexhip;

extern "C" int trexhip_rethreshold_per_blob_device(trexhip_ctx* ctx, int32_t threshold, const int32_t* d_blob_thresholds, int32_t method,
                                                   const double* size_ranges, int32_t n_ranges);

extern "C" {

int trexhip_abi_version(void) { return TREXHIP_ABI_VERSION; }
const char* trexhip_last_error(void) { return g_error.c_str(); }

void trexhip_default_params(trexhip_params* p, int32_t width, int32_t height) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->device = 0;
    p->width = width; p->height = height;
    p->max_batch = 16;
    p->max_runs = 65536;
    p->max_blobs = 2048;
    p->max_pixels = 1 << 20;
    p->threshold = 15; p->threshold_maximum = 255;
    p->enable_difference = 1; p->absolute_difference = 1;
    p->image_invert = 0; p->zero_is_background = 1;
    // keep iff |diff| >= detect_threshold: the rule the reference documents for the detect stage (core/default_config.cpp:1168,
    // docs/parameters_trex.rst:624-629 "disregards any pixel |p| < threshold") in the words of the track-stage rule (:1167), which
    // Tests/test_pixels.cpp:1026-1059 pins as >=.  0 selects the strict comparison (cv::threshold's THRESH_BINARY).
    p->inclusive = 1;
    p->connectivity = 8;
    p->dilation_size = 0; p->use_closing = 0; p->closing_size = 3;
    p->n_ranges = 0; p->cm_per_pixel = 1.0;
    p->pixel_encoding = TREXHIP_ENC_GRAY;
}

int trexhip_create(const trexhip_params* p, trexhip_ctx** out) {
    if (!p || !out) { set_error("trexhip_create: null argument"); return TREXHIP_E_INVALID; }
    *out = nullptr;
    if (p->width <= 0 || p->height <= 0 || p->width >= 65535 || p->height >= 65535) {
        set_error("trexhip_create: frame size must be in 1..65534 (pv.cpp:601-602)"); return TREXHIP_E_INVALID;
    }
    if (p->max_batch <= 0 || p->max_runs <= 0 || p->max_blobs <= 0 || p->max_pixels <= 0) {
        set_error("trexhip_create: capacities must be positive"); return TREXHIP_E_INVALID;
    }
    if ((uint64_t)p->max_batch * (uint64_t)p->max_pixels > 0xffffffffull || (uint64_t)p->max_batch * (uint64_t)p->max_runs > 0xffffffffull ||
        (uint64_t)p->max_batch * (uint64_t)p->max_blobs > 0xffffffffull) {
        set_error("trexhip_create: max_batch * max_pixels / max_runs / max_blobs must stay below 2^32 (pooled tables are indexed with 32 bits)"); return TREXHIP_E_INVALID;
    }
    if (p->connectivity != 8 && p->connectivity != 4) { set_error("trexhip_create: connectivity must be 4 or 8"); return TREXHIP_E_INVALID; }
    {   // settings of the reference that are not implemented: refuse, never diverge silently
        const struct { int32_t v; const char* name; } off[] = {{p->image_adjust, "image_adjust"}, {p->blur_difference, "blur_difference"},
            {p->equalize_histogram, "equalize_histogram"}, {p->correct_luminance, "correct_luminance"}, {p->use_adaptive_threshold, "use_adaptive_threshold"}};
        for (const auto& o : off)
            if (o.v != 0) {
                set_error(std::string("trexhip_create: ") + o.name + " is not implemented by this backend (RawProcessing's optional pre-processing); switch it off or use the CPU detector");
                return TREXHIP_E_UNSUPPORTED;
            }
    }
    if (p->n_ranges < 0 || p->n_ranges > 8) { set_error("trexhip_create: n_ranges must be 0..8"); return TREXHIP_E_INVALID; }
    if ((p->use_closing && (p->closing_size < 1 || p->closing_size > 15)) || p->dilation_size > 7 || p->dilation_size < -7) {
        set_error("trexhip_create: structuring elements larger than 15x15 are not supported (closing_size <= 15, |dilation_size| <= 7)");
        return TREXHIP_E_UNSUPPORTED;
    }
    if (p->pixel_encoding < 0 || p->pixel_encoding > 2) { set_error("trexhip_create: pixel_encoding must be TREXHIP_ENC_GRAY / R3G3B2 / RGB8"); return TREXHIP_E_INVALID; }
    if (p->pixel_encoding != TREXHIP_ENC_GRAY && p->image_invert) {
        set_error("trexhip_create: image_invert with a colour pixel_encoding is not supported"); return TREXHIP_E_UNSUPPORTED;
    }
    int ndev = 0;
    TH_CHECK_HIP(hipGetDeviceCount(&ndev));
    if (p->device < 0 || p->device >= ndev) { set_error("trexhip_create: no such HIP device"); return TREXHIP_E_DEVICE; }
    TH_CHECK_HIP(hipSetDevice(p->device));
    trexhip_ctx* ctx = new (std::nothrow) trexhip_ctx();
    if (!ctx) { set_error("out of host memory"); return TREXHIP_E_NOMEM; }
    ctx->p = *p;
    ctx->pix_ch = p->pixel_encoding == TREXHIP_ENC_RGB8 ? 3 : 1;
    fill_cfg(ctx);
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device) == hipSuccess && cus > 0) ctx->n_cus = cus; }
    // the two test hooks (INTEGRATION.md "Environment variables"): each chooses between schedules that give identical results.
    // TREXHIP_CONV_GEOM: which chain of the identity network runs and which of its preparations (the bits: GEOM_* in cnn_plan.h).  The other
    // bits mean nothing.
    if (const char* e = std::getenv("TREXHIP_CONV_GEOM")) ctx->tune_conv_geom = std::atoi(e) & GEOM_MASK;
    if (const char* e = std::getenv("TREXHIP_CCL_BANDS")) ctx->tune_ccl_bands = std::atoi(e);     // same tables whatever the bands
    const size_t B = p->max_batch, H = p->height, W = p->width, R = p->max_runs, NB = p->max_blobs, P = p->max_pixels;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); delete ctx; return TREXHIP_E_DEVICE; }
    ctx->stream = ctx->own_stream;
    Mem& m = ctx->mem;
    const char* who = "trexhip_create";
    int rc = m.device(&ctx->d_bg, H * W + 16, who);
#define TRY(x) do { if (rc == TREXHIP_OK) rc = (x); } while (0)
    TRY(m.device(&ctx->d_ctr, B * TREXHIP_CTR_STRIDE + 4, who));
    if (rc == TREXHIP_OK && hipMemset(ctx->d_ctr, 0, sizeof(uint32_t) * (B * TREXHIP_CTR_STRIDE + 4)) != hipSuccess) { set_error("hipMemset of the counters failed"); rc = TREXHIP_E_DEVICE; }   // every pass leaves the counters zero (launch_segment)
    TRY(m.device(&ctx->d_band_fail, B, who));
    if (rc == TREXHIP_OK && hipMemset(ctx->d_band_fail, 0, sizeof(uint32_t) * B) != hipSuccess) { set_error("hipMemset of the band flags failed"); rc = TREXHIP_E_DEVICE; }
    TRY(m.device(&ctx->d_row_off, B * H, who));
    TRY(m.device(&ctx->d_tmp_runs, B * (H * TREXHIP_ROW_SLOT + R), who));
    if (rc == TREXHIP_OK) ctx->tables.d_totals = ctx->d_ctr + B * TREXHIP_CTR_STRIDE;   // the pooled totals live behind the per-frame counters
    TRY(alloc_tables(m, ctx->tables, ctx->label, B, H, R, NB, P, ctx->pix_ch, who));
    ctx->tables.fetched = true;     // no batch yet: nothing waits to be fetched
    if (p->use_closing || p->dilation_size != 0) {
        const size_t WBw = (W + 31) / 32;
        TRY(m.device(&ctx->d_bits[0], B * H * WBw + 4, who));
        TRY(m.device(&ctx->d_bits[1], B * H * WBw + 4, who));
    }
    TRY(m.pinned(&ctx->h_ccl_hint, 2, who));
    if (rc == TREXHIP_OK) ctx->h_ccl_hint[0] = ctx->h_ccl_hint[1] = 0u;
#undef TRY
    if (rc != TREXHIP_OK) { trexhip_destroy(ctx); return rc; }
    *out = ctx;
    return TREXHIP_OK;
}

void trexhip_destroy(trexhip_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->p.device);
    (void)fetch_wait(ctx);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->fetch_ev) hipEventDestroy(ctx->fetch_ev);
    net_free(ctx);
    ctx->pass2.mem.free_all();
    upload_free(ctx);
    ctx->mem.free_all();
    stage_free(ctx);
    if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int trexhip_pixel_channels(trexhip_ctx* ctx) { return ctx ? ctx->pix_ch : 0; }

int trexhip_device_alloc(trexhip_ctx* ctx, size_t bytes, void** out_device_ptr) {
    if (!ctx || !out_device_ptr) { set_error("trexhip_device_alloc: null argument"); return TREXHIP_E_INVALID; }
    *out_device_ptr = nullptr;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    TH_CHECK_HIP(hipMalloc(out_device_ptr, bytes ? bytes : 1));
    return TREXHIP_OK;
}

int trexhip_device_free(trexhip_ctx* ctx, void* device_ptr) {
    if (!ctx) { set_error("null ctx"); return TREXHIP_E_INVALID; }
    if (!device_ptr) return TREXHIP_OK;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    TH_CHECK_HIP(hipFree(device_ptr));
    return TREXHIP_OK;
}

int trexhip_copy_to_host(trexhip_ctx* ctx, void* host_dst, const void* device_src, size_t bytes) {
    if (!ctx || (bytes && (!host_dst || !device_src))) { set_error("trexhip_copy_to_host: null argument"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    if (bytes) TH_CHECK_HIP(hipMemcpyAsync(host_dst, device_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return TREXHIP_OK;
}

int trexhip_copy_to_device(trexhip_ctx* ctx, void* device_dst, const void* host_src, size_t bytes) {
    if (!ctx || (bytes && (!device_dst || !host_src))) { set_error("trexhip_copy_to_device: null argument"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    if (bytes) TH_CHECK_HIP(hipMemcpyAsync(device_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return TREXHIP_OK;
}

int trexhip_get_live_params(trexhip_ctx* ctx, trexhip_live_params* out) {
    if (!ctx || !out) { set_error("trexhip_get_live_params: null argument"); return TREXHIP_E_INVALID; }
    const trexhip_params& p = ctx->p;
    std::memset(out, 0, sizeof(*out));
    out->threshold = p.threshold; out->threshold_maximum = p.threshold_maximum; out->inclusive = p.inclusive;
    out->enable_difference = p.enable_difference; out->absolute_difference = p.absolute_difference;
    out->image_invert = p.image_invert; out->zero_is_background = p.zero_is_background;
    out->n_ranges = p.n_ranges; out->cm_per_pixel = p.cm_per_pixel;
    for (int i = 0; i < 16; ++i) out->ranges[i] = p.ranges[i];
    return TREXHIP_OK;
}

int trexhip_update_params(trexhip_ctx* ctx, const trexhip_live_params* lp) {
    if (!ctx || !lp) { set_error("trexhip_update_params: null argument"); return TREXHIP_E_INVALID; }
    if (lp->n_ranges < 0 || lp->n_ranges > 8) { set_error("trexhip_update_params: n_ranges must be 0..8 (detect_size_filter with more than 8 ranges is not supported)"); return TREXHIP_E_INVALID; }
    if (!(lp->cm_per_pixel > 0.0)) { set_error("trexhip_update_params: cm_per_pixel must be positive"); return TREXHIP_E_INVALID; }
    if (ctx->p.pixel_encoding != TREXHIP_ENC_GRAY && lp->image_invert) {
        set_error("trexhip_update_params: image_invert with a colour pixel_encoding is not supported"); return TREXHIP_E_UNSUPPORTED;
    }
    trexhip_params& p = ctx->p;
    p.threshold = lp->threshold; p.threshold_maximum = lp->threshold_maximum; p.inclusive = lp->inclusive;
    p.enable_difference = lp->enable_difference; p.absolute_difference = lp->absolute_difference;
    p.image_invert = lp->image_invert; p.zero_is_background = lp->zero_is_background;
    p.n_ranges = lp->n_ranges; p.cm_per_pixel = lp->cm_per_pixel;
    for (int i = 0; i < 16; ++i) p.ranges[i] = i < 2 * lp->n_ranges ? lp->ranges[i] : 0.0;
    return fill_cfg(ctx);
}

int trexhip_set_stream(trexhip_ctx* ctx, void* hip_stream) {
    if (!ctx) { set_error("null ctx"); return TREXHIP_E_INVALID; }
    // (with the table copies of trexhip_fetch_begin pending on the stream that is left -- fetch_begin synchronised it in front of them --, they
    // stay there behind their event: trexhip_fetch_wait waits for them, not this call)
    if (!(ctx->fetch_pending && ctx->fetch_stream == ctx->stream)) TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return TREXHIP_OK;
}

int trexhip_set_background(trexhip_ctx* ctx, const uint8_t* gray, int32_t stride) {
    if (!ctx || !gray) { set_error("trexhip_set_background: null argument"); return TREXHIP_E_INVALID; }
    if (stride < ctx->p.width) { set_error("trexhip_set_background: stride < width"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    TH_CHECK_HIP(hipMemcpy2DAsync(ctx->d_bg, ctx->p.width, gray, stride, ctx->p.width, ctx->p.height,
                                  hipMemcpyHostToDevice, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->has_bg = true;
    return TREXHIP_OK;
}

int trexhip_set_background_device(trexhip_ctx* ctx, const uint8_t* d_gray) {
    if (!ctx || !d_gray) { set_error("trexhip_set_background_device: null argument"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    TH_CHECK_HIP(hipMemcpyAsync(ctx->d_bg, d_gray, (size_t)ctx->p.width * ctx->p.height, hipMemcpyDeviceToDevice, ctx->stream));
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    ctx->has_bg = true;
    return TREXHIP_OK;
}

static int check_segment_args(trexhip_ctx* ctx, const void* frames, int32_t n) {
    if (!ctx || !frames) { set_error("trexhip_segment: null argument"); return TREXHIP_E_INVALID; }
    if (!ctx->has_bg) { set_error("trexhip_segment: background image not set"); return TREXHIP_E_INVALID; }
    if (n < 0 || n > ctx->p.max_batch) { set_error("trexhip_segment: n outside 0..max_batch"); return TREXHIP_E_INVALID; }
    return TREXHIP_OK;
}

int trexhip_segment_device(trexhip_ctx* ctx, const uint8_t* d_frames, int32_t n) {
    int rc = check_segment_args(ctx, d_frames, n);
    if (rc) return rc;
    if (ctx->pix_ch != 1 || ctx->p.pixel_encoding != TREXHIP_ENC_GRAY) { set_error("trexhip_segment_device: a colour pixel_encoding needs colour input (trexhip_segment_color*)"); return TREXHIP_E_INVALID; }
    ctx->d_color_src = nullptr; ctx->color_ch = 0;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    if (n == 0) { ctx->tables.valid_n = 0; ctx->tables.fetched = false; return TREXHIP_OK; }
    return launch_segment(ctx, d_frames, n);
}

int trexhip_segment(trexhip_ctx* ctx, const uint8_t* const* frames, int32_t stride, int32_t n) {
    int rc = check_segment_args(ctx, frames, n);
    if (rc) return rc;
    if (ctx->p.pixel_encoding != TREXHIP_ENC_GRAY) { set_error("trexhip_segment: a colour pixel_encoding needs colour input (trexhip_segment_color*)"); return TREXHIP_E_INVALID; }
    ctx->d_color_src = nullptr; ctx->color_ch = 0;
    if (stride < ctx->p.width) { set_error("trexhip_segment: stride < width"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    if (n == 0) { ctx->tables.valid_n = 0; ctx->tables.fetched = false; return TREXHIP_OK; }
    const size_t W = ctx->p.width, H = ctx->p.height;
    rc = ensure_staging(ctx, "trexhip_segment");
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (!frames[i]) { set_error("trexhip_segment: null frame pointer"); return TREXHIP_E_INVALID; }
    // pageable frame -> pinned ring slot (host threads) -> HBM, one async DMA per frame overlapping the next frame's staging (upload.hip)
    rc = upload_frames(ctx, frames, n, H, W, (size_t)stride, ctx->d_staging, nullptr);
    if (rc) return rc;
    return launch_segment(ctx, ctx->d_staging, n);
}

int trexhip_synchronize(trexhip_ctx* ctx) {
    if (!ctx) { set_error("null ctx"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return TREXHIP_OK;
}


}  // extern "C"
namespace trexhip {
// A batch of a few frames (TRex's default detect_batch_size is ONE frame per call) leaves the device as ONE launch that writes the frame table, the
// totals and exactly the filled parts of the blob / line / pixel tables into the context's pinned host mirrors, followed by ONE stream synchronize.
// The DMA path below needs two round trips (frame table and totals first, then three copies whose sizes the totals give): five small copies with
// 10-17 us of host latency between them -- more than the detect kernels of one frame take (profiles/r06_batch1_timeline.txt).  4-byte words: every
// table is a multiple of 4 bytes except the pixels, whose tail bytes go out one by one.
__global__ __launch_bounds__(256) void k_export(const trexhip_frame_info* __restrict__ info, const uint32_t* __restrict__ totals,
                                                const trexhip_blob* __restrict__ blobs, const trexhip_run* __restrict__ runs, const uint8_t* __restrict__ pixels,
                                                trexhip_frame_info* __restrict__ h_info, uint32_t* __restrict__ h_totals, trexhip_blob* __restrict__ h_blobs,
                                                trexhip_run* __restrict__ h_runs, uint8_t* __restrict__ h_pixels, const int n,
                                                const uint32_t pool_blobs, const uint32_t pool_runs, const uint32_t pool_pixels, const int pix_ch) {
    const uint32_t tb = min(totals[0], pool_blobs), tr = min(totals[1], pool_runs), tp = min(totals[2], pool_pixels);
    const size_t gtid = (size_t)blockIdx.x * 256 + threadIdx.x, gstep = (size_t)gridDim.x * 256;
    auto words = [&](const void* src, void* dst, const size_t nw) {
        const uint32_t* a = static_cast<const uint32_t*>(src);
        uint32_t* b = static_cast<uint32_t*>(dst);
        for (size_t i = gtid; i < nw; i += gstep) b[i] = a[i];
    };
    words(info, h_info, (size_t)n * sizeof(trexhip_frame_info) / 4);
    if (gtid < 4) h_totals[gtid] = totals[gtid];
    words(blobs, h_blobs, (size_t)tb * sizeof(trexhip_blob) / 4);
    words(runs, h_runs, (size_t)tr * sizeof(trexhip_run) / 4);
    const size_t pb = (size_t)tp * pix_ch;
    words(pixels, h_pixels, pb / 4);
    if (gtid < (pb & 3)) h_pixels[(pb & ~(size_t)3) + gtid] = pixels[(pb & ~(size_t)3) + gtid];
}
static_assert(sizeof(trexhip_frame_info) % 4 == 0 && sizeof(trexhip_blob) % 4 == 0 && sizeof(trexhip_run) % 4 == 0, "k_export copies 4-byte words");
static constexpr int EXPORT_MAX_FRAMES = 16;
// frame table and totals into the pinned mirrors, and with n <= EXPORT_MAX_FRAMES the filled parts of the three tables along with them
static int export_or_fetch_info(trexhip_ctx* ctx, bool by_kernel) {
    BlobTables& t = ctx->tables;
    if (!by_kernel) return fetch_info(ctx, t);
    hipLaunchKernelGGL(k_export, dim3(32), dim3(256), 0, ctx->stream, t.d_info, t.d_totals, t.d_blobs, t.d_runs, t.d_pixels, t.h_info, t.h_totals, t.h_blobs,
                       t.h_runs, t.h_pixels, t.valid_n, ctx->cfg.pool_blobs, ctx->cfg.pool_runs, ctx->cfg.pool_pixels, ctx->pix_ch);
    TH_CHECK_HIP(hipGetLastError());
    TH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return TREXHIP_OK;
}
}  // namespace trexhip
extern "C" {

// trexhip_fetch, or (begin) everything of it but the wait for the three table copies of a batch that k_export does not serve
static int fetch_batch(trexhip_ctx* ctx, trexhip_batch_result* out, const char* who, const bool begin) {
    if (!ctx || !out) { set_error(std::string(who) + ": null argument"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    if (const int rc = fetch_wait(ctx)) return rc;      // (copies still on their way write the mirrors this call fills)
    BlobTables& t = ctx->tables;
    const int n = t.valid_n;
    const bool by_kernel = n <= EXPORT_MAX_FRAMES;      // a few frames: one launch + one synchronize (k_export)
    if (n) {
        int rc1 = export_or_fetch_info(ctx, by_kernel);
        if (rc1) return rc1;
        bool pending = false;
        for (int i = 0; i < n; ++i) pending |= t.h_info[i].reserved[0] == 1u;
        if (pending) {   // frames with more runs than fit in LDS: finish them with the global-memory chain
            rc1 = launch_pending(ctx);
            if (rc1 == TREXHIP_OK) rc1 = export_or_fetch_info(ctx, by_kernel);
            if (rc1) return rc1;
        }
    }
    int rc = fetch_tables(ctx, t, !by_kernel, out, begin);
    if (rc || n == 0) return rc;
    for (int i = 0; i < n; ++i)
        if (t.h_info[i].flags & TREXHIP_FRAME_MALFORMED) {       // a loaded frame (trexhip_load_frames_v6_device) that broke a rule of pv_read.h
            char buf[160];
            std::snprintf(buf, sizeof(buf), "frame %d of the batch is malformed: its V_6 body breaks the layout (flags=%u); it holds no blobs", i, t.h_info[i].flags);
            set_error(buf);
            return TREXHIP_E_INVALID;
        }
    for (int i = 0; i < n; ++i)
        if (t.h_info[i].flags) {
            char buf[160];
            std::snprintf(buf, sizeof(buf), "frame %d of the batch exceeded capacity (flags=%u, raw runs=%u): raise max_runs/max_blobs/max_pixels",
                          i, t.h_info[i].flags, t.h_info[i].n_raw_runs);
            set_error(buf);
            rc = TREXHIP_E_CAPACITY;
        }
    return rc;
}

int trexhip_fetch(trexhip_ctx* ctx, trexhip_batch_result* out) { return fetch_batch(ctx, out, "trexhip_fetch", false); }
int trexhip_fetch_begin(trexhip_ctx* ctx, trexhip_batch_result* out) { return fetch_batch(ctx, out, "trexhip_fetch_begin", true); }
int trexhip_fetch_wait(trexhip_ctx* ctx) {
    if (!ctx) { set_error("trexhip_fetch_wait: null ctx"); return TREXHIP_E_INVALID; }
    return fetch_wait(ctx);
}

static int pass2_alloc(trexhip_ctx* ctx, const char* who) {
    Pass2& q = ctx->pass2;
    if (q.allocated) return TREXHIP_OK;
    const size_t B = ctx->p.max_batch, R = ctx->p.max_runs;
    int rc = alloc_tables(q.mem, q.tables, q.label, B, ctx->p.height, R, ctx->p.max_blobs, ctx->p.max_pixels, ctx->pix_ch, who);
    if (rc == TREXHIP_OK) rc = q.mem.device(&q.d_sub_cnt, B * R, who);
    if (rc == TREXHIP_OK) rc = q.mem.device(&q.d_sub_base, B * R, who);
    if (rc == TREXHIP_OK) rc = q.mem.device(&q.d_run_parent, B * R, who);
    if (rc != TREXHIP_OK) { q.mem.free_all(); q = Pass2(); }
    q.allocated = rc == TREXHIP_OK;
    return rc;
}

int trexhip_rethreshold_device(trexhip_ctx* ctx, int32_t threshold, int32_t method, const double* size_ranges, int32_t n_ranges) {
    return trexhip_rethreshold_per_blob_device(ctx, threshold, nullptr, method, size_ranges, n_ranges);
}

int trexhip_rethreshold_per_blob_device(trexhip_ctx* ctx, int32_t threshold, const int32_t* d_blob_thresholds, int32_t method,
                                        const double* size_ranges, int32_t n_ranges) {
    int rc = trexhip::rethreshold_prepare(ctx, "trexhip_rethreshold_device", method, size_ranges, n_ranges);
    if (rc) return rc;
    return launch_rethreshold(ctx, threshold, method, size_ranges, n_ranges, d_blob_thresholds);
}

int trexhip_fetch_rethreshold(trexhip_ctx* ctx, trexhip_batch_result* out) {
    if (!ctx || !out) { set_error("trexhip_fetch_rethreshold: null argument"); return TREXHIP_E_INVALID; }
    Pass2& q = ctx->pass2;
    if (!q.allocated || q.tables.valid_n == 0) { set_error("trexhip_fetch_rethreshold: no re-thresholded batch"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    const int n = q.tables.valid_n;
    int rc = fetch_info(ctx, q.tables);
    if (rc == TREXHIP_OK) rc = fetch_tables(ctx, q.tables, true, out);
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (q.tables.h_info[i].flags) { set_error("a frame exceeded capacity during re-threshold: raise max_runs/max_blobs/max_pixels"); return TREXHIP_E_CAPACITY; }
    return TREXHIP_OK;
}

int trexhip_device_view_get(trexhip_ctx* ctx, trexhip_device_view* out) {
    if (!ctx || !out) { set_error("trexhip_device_view_get: null argument"); return TREXHIP_E_INVALID; }
    out->frames = ctx->tables.d_info; out->blobs = ctx->tables.d_blobs; out->runs = ctx->tables.d_runs; out->pixels = ctx->tables.d_pixels;
    out->totals = ctx->tables.d_totals; out->blob_frame = ctx->tables.d_blob_frame;
    return TREXHIP_OK;
}

int trexhip_profile_enable(trexhip_ctx* ctx, int32_t on) {
    if (!ctx) { set_error("null ctx"); return TREXHIP_E_INVALID; }
    ctx->profiling = on != 0;
    return TREXHIP_OK;
}

int trexhip_profile_read(trexhip_ctx* ctx, int32_t stage, double* total_ms, int64_t* launches) {
    if (!ctx || stage < 0 || stage >= TREXHIP_STAGE_COUNT) { set_error("trexhip_profile_read: bad argument"); return TREXHIP_E_INVALID; }
    if (stage == TREXHIP_STAGE_UPLOAD_COPY || stage == TREXHIP_STAGE_UPLOAD_DMA) {     // host-input legs (upload.hip), per frame
        Uploader& u = ctx->up;
        if (stage == TREXHIP_STAGE_UPLOAD_DMA)
            for (int k = 0; k < UP_SLOTS; ++k)
                if (u.busy[k] && hipEventQuery(u.ev_done[k]) == hipSuccess) {
                    float ms = 0.f;
                    if (hipEventElapsedTime(&ms, u.ev_start[k], u.ev_done[k]) == hipSuccess) { u.dma_ms += ms; u.dma_n += u.frames_in[k]; }
                    u.busy[k] = false;
                }
        if (total_ms) *total_ms = stage == TREXHIP_STAGE_UPLOAD_COPY ? u.copy_ms : u.dma_ms;
        if (launches) *launches = stage == TREXHIP_STAGE_UPLOAD_COPY ? u.copy_n : u.dma_n;
        return TREXHIP_OK;
    }
    stage_read(ctx, stage);
    Stage& s = ctx->stages[stage];
    if (total_ms) *total_ms = s.total_ms;
    if (launches) *launches = s.launches;
    return TREXHIP_OK;
}

int trexhip_profile_reset(trexhip_ctx* ctx) {
    if (!ctx) { set_error("null ctx"); return TREXHIP_E_INVALID; }
    for (int i = 0; i < TREXHIP_STAGE_COUNT; ++i) { stage_read(ctx, i); ctx->stages[i].total_ms = 0.0; ctx->stages[i].launches = 0; }
    for (int k = 0; k < UP_SLOTS; ++k)                       // uploads still in flight belong to the period before the reset
        if (ctx->up.busy[k]) { (void)hipEventSynchronize(ctx->up.ev_done[k]); ctx->up.busy[k] = false; }
    ctx->up.copy_ms = ctx->up.dma_ms = 0.0; ctx->up.copy_n = ctx->up.dma_n = 0;
    return TREXHIP_OK;
}

}  // extern "C"

namespace trexhip {
// what every entry point that runs the re-threshold pass checks before it launches: arguments, a fetched batch, the second table set
int rethreshold_prepare(trexhip_ctx* ctx, const char* who, int32_t method, const double* size_ranges, int32_t n_ranges) {
    const std::string w(who);
    if (!ctx) { set_error(w + ": null ctx"); return TREXHIP_E_INVALID; }
    if (method < 0 || method > 2) { set_error(w + ": method must be 0 (absolute), 1 (sign) or 2 (none)"); return TREXHIP_E_INVALID; }
    if (n_ranges < 0 || n_ranges > 8 || (n_ranges && !size_ranges)) { set_error(w + ": bad size ranges"); return TREXHIP_E_INVALID; }
    if (!ctx->d_frames || ctx->tables.valid_n == 0) { set_error(w + ": no segmented batch"); return TREXHIP_E_INVALID; }
    if (!ctx->tables.fetched) { set_error(w + ": call trexhip_fetch on the segmented batch first"); return TREXHIP_E_INVALID; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    return pass2_alloc(ctx, who);
}
}
