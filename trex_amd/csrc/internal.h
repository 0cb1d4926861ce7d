// internal.h -- shared declarations of libtrexhip (not part of the ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <string>
#include <vector>
#include "../../include/trexhip.h"
#include "cnn_prepared.h"

#define TREXHIP_ROW_SLOT 16
#define TREXHIP_CTR_STRIDE 32

namespace trexhip {

void set_error(const std::string& msg);

#define TH_CHECK_HIP(expr)                                                                    \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::trexhip::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));          \
            return TREXHIP_E_DEVICE;                                                          \
        }                                                                                     \
    } while (0)

// wave-uniform constants handed to every segment kernel by value
struct SegCfg {
    int W, H, B;          // frame size, frames in this launch
    int ctr_frames;       // frames the per-frame counter array was sized for (max_batch): the pooled totals live behind them
    int R;                // raw run capacity per frame
    int T;                // entries per frame in the tmp run array = H*ROW_SLOT + R
    int tmin;             // smallest difference value that passes the threshold
    int tmax;             // largest passing value (255 unless threshold_maximum < 255)
    int enable_diff, absdiff, invert, zero_bg;
    int slack;            // 1 for 8-connectivity, 0 for 4
    int n_ranges;
    float sqcm;
    double ranges[16];
    uint32_t pool_blobs, pool_runs, pool_pixels;
    uint32_t cap_blobs, cap_pixels;   // per frame (max_blobs, max_pixels): a frame beyond them fails alone, before it reserves pooled space
};

// live kernel timing: event pairs are recorded on the ctx stream and only read (folded) on
// trexhip_profile_read, so enabling profiling never adds a host sync to the timed region
struct EvPair { hipEvent_t a = nullptr, b = nullptr; };
struct Stage {
    std::vector<EvPair> pending, freelist;
    EvPair cur;
    double total_ms = 0.0;
    int64_t launches = 0;
};

}  // namespace trexhip

namespace trexhip {
// every device and pinned-host allocation of a context, a network or a trainer is handed out here, remembered, and freed in one call (mem.hip).
// A count of 0 is treated as 1.  A failed allocation is reported the same way everywhere: out of memory is TREXHIP_E_NOMEM with a message that
// names the entry point (`who`), any other HIP failure TREXHIP_E_DEVICE.
struct Mem {
    std::vector<void*> dev, host;
    int alloc(void** p, size_t bytes, bool pinned, const char* who);
    template <typename T> int device_bytes(T** p, size_t bytes, const char* who) { return alloc(reinterpret_cast<void**>(p), bytes, false, who); }
    template <typename T> int device(T** p, size_t count, const char* who) { return device_bytes(p, (count ? count : 1) * sizeof(T), who); }
    template <typename T> int pinned(T** p, size_t count, const char* who) { return alloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T), true, who); }
    void release(void* d);      // one device buffer ahead of the rest (Scratch::reserve)
    void free_all();
};

// a grow-on-demand device buffer of the context, sized in bytes.  reserve() does nothing while the buffer is large enough; otherwise it waits for
// the context's stream (an earlier call may still read the old buffer), frees it and allocates `need` bytes from ctx->mem.
struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    int reserve(trexhip_ctx* ctx, size_t need, const char* who);
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// the pooled output tables of one CCL pass and their pinned host mirrors
struct BlobTables {
    trexhip_frame_info* d_info = nullptr;  // [B]
    trexhip_blob* d_blobs = nullptr;       // [B*NB] pooled
    uint32_t* d_blob_frame = nullptr;      // [B*NB]
    trexhip_run* d_runs = nullptr;         // [B*R] pooled, grouped by blob
    uint8_t* d_pixels = nullptr;           // [B*P*pix_ch] pooled
    uint32_t* d_totals = nullptr;          // [4] pooled totals: blobs, runs, pixels (pass 1: the words behind ctx->d_ctr's per-frame counters)
    trexhip_frame_info* h_info = nullptr;
    uint32_t* h_totals = nullptr;
    trexhip_blob* h_blobs = nullptr;
    trexhip_run* h_runs = nullptr;
    uint8_t* h_pixels = nullptr;
    int valid_n = 0;                       // frames of the batch the device tables hold
    bool fetched = false;                  // the host mirrors hold that batch
};
// the per-run labelling arrays of one CCL pass
struct LabelState {
    uint32_t* d_row_cnt = nullptr;      // [B*H]
    uint32_t* d_row_base = nullptr;     // [B*(H+1)] exclusive scan of row_cnt = raster index
    trexhip_run* d_raster = nullptr;    // [B*R]   runs in raster order
    uint32_t* d_parent = nullptr;       // [B*R]   union-find parent -> root label
    uint32_t* d_root_ord = nullptr;     // [B*R]   ordinal of the raw blob rooted at run r
    uint32_t* d_cnt_runs = nullptr;     // [B*R]   per raw blob
    uint32_t* d_cnt_px = nullptr;       // [B*R]
    uint32_t* d_cur_run = nullptr;      // [B*R]   frame-relative run cursor per raw blob
    uint32_t* d_pix_begin = nullptr;    // [B*R]   frame-relative pixel begin per raw blob
    int32_t* d_blob_map = nullptr;      // [B*R]   raw blob ordinal -> kept index or -1
};
// second CCL pass (track-stage re-threshold): its own tables and labelling state, allocated on first use
struct Pass2 {
    bool allocated = false;
    Mem mem;
    BlobTables tables;
    LabelState label;
    uint32_t *d_sub_cnt = nullptr, *d_sub_base = nullptr, *d_run_parent = nullptr;   // [B*R]
};
}

namespace trexhip {
// host tiles -> HBM (upload.hip): ring of pinned slots, copy stream, host copy threads, timings of the two legs
enum { UP_SLOTS = 3 };
static constexpr size_t UP_CHUNK_BYTES = (size_t)32 << 20;   // frames per DMA: about this many bytes
struct Uploader {
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_start[UP_SLOTS] = {}, ev_done[UP_SLOTS] = {};
    bool busy[UP_SLOTS] = {};
    int frames_in[UP_SLOTS] = {};
    uint8_t* ring = nullptr;            // UP_SLOTS x slot_bytes, pinned
    size_t slot_bytes = 0;
    void* pool = nullptr;               // CopyPool
    double copy_ms = 0.0, dma_ms = 0.0;
    int64_t copy_n = 0, dma_n = 0;
};
}

struct trexhip_ctx {
    trexhip_params p;
    trexhip::SegCfg cfg;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool has_bg = false;
    int batch_invert = 0, batch_zero_bg = 0;      // image_invert / zero_is_background the LAST segmented batch was taken with: its crops, re-threshold and
                                                  // split search keep them although trexhip_update_params may have changed the live settings since

    // device memory (layout: DESIGN.md "Data layout in HBM")
    trexhip::Mem mem;                   // owns every buffer below
    trexhip::BlobTables tables;         // pass 1: valid_n frames of the last segmented / loaded batch
    // trexhip_fetch_begin: the copies of the three pooled tables into the pinned mirrors are queued, fetch_ev is recorded behind them on
    // fetch_stream, and nobody has waited for it yet (trexhip::fetch_wait)
    hipEvent_t fetch_ev = nullptr;      // created on first use, hipEventDisableTiming
    hipStream_t fetch_stream = nullptr;
    bool fetch_pending = false;
    trexhip::LabelState label;
    uint8_t* d_bg = nullptr;
    uint8_t* d_staging = nullptr;       // frames uploaded by the host-pointer API
    const uint8_t* d_frames = nullptr;  // frames of the last segment call
    uint32_t* d_ctr = nullptr;          // [B*CTR_STRIDE] per-frame overflow counters (128 B apart) + [4] pooled totals (tables.d_totals)
    uint32_t* d_band_fail = nullptr;    // [B] a band of the frame held more lines than k_ccl_band's workgroup takes (k_ccl_lds reads and clears it)
    uint32_t* d_row_off = nullptr;      // [B*H]   offset of the row's runs in tmp order
    uint32_t* d_tmp_runs = nullptr;     // [B*T]   x0 | x1 << 16; T = H*ROW_SLOT (row slots) + R (overflow area)
    // grown on demand
    trexhip::Scratch warp;              // double[6] per blob: inverse affine maps of the normalised crops
    trexhip::Scratch len;               // float per blob: (median) midline lengths handed in by the caller (midline.hip); u64 per frame: timestamps (pack.hip)
    trexhip::Scratch aug_idx;           // int32: index list of the last trexhip_augment_device call (copied in stream order, so one buffer serves every call)
    trexhip::Scratch val;               // scratch and results of trexhip_validation_metrics_device (validate.hip)
    trexhip::Scratch avg;               // scratch and results of trexhip_class_averages_device (averages.hip)
    trexhip::Scratch vf;                // scratch of trexhip_visual_field_device (visual_field.hip): flag, tessellated outlines
    trexhip::Scratch autos;             // scratch of trexhip_posture_auto_device (thresholds, selections, first outlines)
    trexhip::Scratch pre;               // second counts and sequence scratch of trexhip_prefilter_device (prefilter.hip), fixed size
    trexhip::Scratch load;              // blob index and frame counts of trexhip_load_frames_v6_device (unpack.hip), fixed size
    trexhip::Scratch bg_color;          // colour background ([H][W][bg_color_ch]) for the difference crops of the rgb8 encoding
    uint32_t* d_bits[2] = {nullptr, nullptr};   // 1 bit/pixel masks for the optional morphology [B][H][ceil(W/32)]
    uint8_t* d_color = nullptr;         // BGR/BGRA frames of the colour-input API

    void* net = nullptr;                // trexhip::Net (cnn.hip)
    void* cat = nullptr;                // trexhip::Net of the category network (cnn_arch.hip), beside the identity network: neither load touches the other
    trexhip::Scratch vote;              // flag, skipped count of trexhip_tracklet_labels_device (categorize.hip)
    trexhip::Scratch med;               // flags, counts, offsets and row list of trexhip_tracklet_medians_device (tracklet_median.hip)
    trexhip::Pass2 pass2;
    int cnn_mode = TREXHIP_CNN_FP16X3;  // TREXHIP_CNN_*: fp32-class arithmetic on the fp16 matrix cores, range-guarded
    trexhip::PreparedState prepared;    // what trexhip_identify_prepare_device queued for the next identify call (cnn_prepared.h)

    bool profiling = false;
    int tune_conv_geom = 0;             // dev only: which identity-network chain runs (TREXHIP_CONV_GEOM, bits 0-11 and 23-30)
    // hipFuncSetAttribute is per device: one process may drive several devices through several contexts
    bool attr_cnn = false, attr_ccl = false, attr_split = false, attr_prefilter = false;
    bool ctr_dirty = false;             // a detect pass was queued but not to its end: the per-frame overflow counters may be non-zero (launch_segment zeroes them first)
    int attr_posture_bytes = 0;
    int pix_ch = 1;                     // bytes per output pixel (pixel_encoding)
    const uint8_t* d_color_src = nullptr; // colour frames of the last segment_color* call ([n][H][W][color_ch])
    int color_ch = 0;
    int bg_color_ch = 0;
    int n_cus = 256;                    // compute units of the device (persistent kernels size their grids with it)
    int tune_ccl_bands = -1;            // test hook: several workgroups per frame (TREXHIP_CCL_BANDS; -1 = by the frames per launch and the hint word, 0 never, n always n bands)
    uint32_t* h_ccl_hint = nullptr;     // [2] pinned, written by k_ccl_lds: a frame had more lines than the S / the M instance holds
    uint32_t ccl_calls = 0;
    trexhip::Stage stages[TREXHIP_STAGE_COUNT];
    trexhip::Uploader up;
};

namespace trexhip {
int launch_segment(trexhip_ctx* ctx, const uint8_t* d_frames, int n);
void stage_begin(trexhip_ctx* ctx, int stage);
void stage_end(trexhip_ctx* ctx, int stage);
void net_free(trexhip_ctx* ctx);
// blocks until the table copies of a trexhip_fetch_begin have arrived; at once with nothing pending.  Called by every entry point that overwrites
// the device tables or the pinned mirrors, or reads the mirrors on the host (capi.hip)
int fetch_wait(trexhip_ctx* ctx);
int launch_pending(trexhip_ctx* ctx);
int launch_morphology(trexhip_ctx* ctx, const uint8_t* d_frames, int n, const uint32_t** result);
int launch_rethreshold(trexhip_ctx* ctx, int thr, int method, const double* ranges, int n_ranges, const int32_t* d_blob_thr);
// the checks shared by every entry point that runs the re-threshold pass (arguments, a fetched batch) + the second table set on first use (capi.hip)
int rethreshold_prepare(trexhip_ctx* ctx, const char* who, int32_t method, const double* size_ranges, int32_t n_ranges);
int launch_prefilter(trexhip_ctx* ctx, const trexhip_prefilter_params* pp, const trexhip_prefilter_tables* tb, uint8_t* d_decision, int32_t* d_order,
                     int32_t* d_counts, int32_t* d_presumed_nr);
int launch_to_gray(trexhip_ctx* ctx, const uint8_t* d_color, uint8_t* d_gray, size_t npix, int channels, int color_channel);
int ensure_staging(trexhip_ctx* ctx, const char* who);   // ctx->d_staging, allocated on first use (mem.hip)
void upload_free(trexhip_ctx* ctx);
int upload_frames(trexhip_ctx* ctx, const uint8_t* const* frames, int n, size_t rows, size_t row_bytes, size_t stride, uint8_t* d_dst,
                  const std::function<int(int, int)>& after_chunk, int reduce_channels = 0, int color_channel = -1);
}
