/*
 * trexhip.h -- C ABI of libtrexhip: the MI355X (gfx950) implementation of TRex's per-frame
 * detection + identity hot path.  extern "C", plain pointers and sizes only.
 *
 * Each entry point names the reference interface (file:line under /root/reference) whose work
 * it replaces; INTEGRATION.md shows the binding a TRex maintainer adds on the C++ side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative TREXHIP_E_* code; the message is kept
 *     per thread and read with trexhip_last_error().  No exception crosses this ABI.
 *   - one ctx per (host thread, device); calls on one ctx are not re-entrant.
 *   - "_device" variants take device pointers (HBM-resident data) and only enqueue work on the
 *     ctx stream; the plain variants take host pointers and include the PCIe copies.
 *   - all result pointers handed out stay owned by the ctx and are valid until the next call
 *     of the same function on that ctx.
 */
#ifndef TREXHIP_H
#define TREXHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TREXHIP_ABI_VERSION 27

/* A failed allocation is reported the same way by every entry point: when the device (or the pinned host pool) is out of memory the call
   returns TREXHIP_E_NOMEM and trexhip_last_error() names the entry point; any other HIP failure is TREXHIP_E_DEVICE.  (Up to and including
   the first release of ABI 13 some entry points returned TREXHIP_E_DEVICE for an exhausted device.) */
enum {
    TREXHIP_OK = 0,
    TREXHIP_E_INVALID = -1,    /* bad argument / not initialised (e.g. no background yet)   */
    TREXHIP_E_DEVICE = -2,     /* HIP runtime error                                         */
    TREXHIP_E_CAPACITY = -3,   /* a frame exceeded max_runs / pooled output capacity         */
    TREXHIP_E_UNSUPPORTED = -4, /* a setting of the reference that this library does not implement was switched on   */
    TREXHIP_E_NOMEM = -5
};

/* per-frame status bits in trexhip_frame_info.flags */
#define TREXHIP_FRAME_OVERFLOW_RUNS   1u
#define TREXHIP_FRAME_OVERFLOW_OUTPUT 2u
#define TREXHIP_FRAME_MALFORMED       4u   /* trexhip_load_frames_v6_device: the frame's stored body breaks the V_6 layout; it holds no blobs */

/* Settings the hot path reads (names = TRex setting names). */
typedef struct trexhip_params {
    int32_t device;              /* HIP device ordinal                                         */
    int32_t width, height;       /* frame size in pixels, < 65535 (pv.cpp:601-602)             */
    int32_t max_batch;           /* frames per segment call                                    */
    int32_t max_runs;            /* capacity: raw horizontal lines per frame                   */
    int32_t max_blobs;           /* capacity: kept blobs per frame (pool = max_batch * this)   */
    int32_t max_pixels;          /* capacity: kept foreground pixels per frame (pooled)        */
    /* RawProcessing::generate_binary (BackgroundSubtraction.cpp:209) */
    int32_t threshold;           /* detect_threshold            grabber/misc/default_config.cpp:98  */
    int32_t threshold_maximum;   /* threshold_maximum           :99 (<255 => inRange[thr,max])      */
    int32_t enable_difference;   /* enable_difference           :126                                */
    int32_t absolute_difference; /* detect_threshold_is_absolute core/default_config.cpp:1168       */
    int32_t image_invert;        /* image_invert                :1159                               */
    int32_t inclusive;           /* 1 (default): keep diff >= thr; 0: diff > thr (a plain cv::threshold).  UNPINNED: the detect-stage comparison
                                  * happens inside RawProcessing::generate_binary (BackgroundSubtraction.cpp:209), whose source is not in the
                                  * reference tree.  The default follows the documented wording ("disregards any pixel |p| < threshold",
                                  * core/default_config.cpp:1168 -- the words of the track-stage rule :1167, which Tests/test_pixels.cpp:1026-1059
                                  * pins as >=); the reference's golden CSVs cannot tell the two apart.  A maintainer who
                                  * knows generate_binary to be strict sets 0 here (HipBackgroundSubtraction::Settings::inclusive = false). */
    int32_t zero_is_background;  /* 1 (default): a masked pixel of grey value 0 is background        */
    /* CPULabeling::run (BackgroundSubtraction.cpp:216) */
    int32_t connectivity;        /* 8 (default) or 4                                                 */
    int32_t dilation_size;       /* core/default_config.cpp:1163                                     */
    int32_t use_closing;         /* :1164                                                            */
    int32_t closing_size;        /* :1165                                                            */
    /* size filter (BackgroundSubtraction.cpp:259, core/SizeFilters.cpp:37-53) */
    int32_t n_ranges;            /* detect_size_filter, 0 = accept all                               */
    double  cm_per_pixel;
    double  ranges[16];          /* [start,end) pairs in cm^2                                        */
    /* meta_encoding of the produced pixel arrays (Background::meta_encoding(), BackgroundSubtraction.cpp:132,151-186):
     * TREXHIP_ENC_GRAY 1 B/px grey value; TREXHIP_ENC_R3G3B2 1 B/px colour code (convert_to_r3g3b2, layout pinned by
     * Tests/test_pixels.cpp:629-795); TREXHIP_ENC_RGB8 3 B/px in the input's memory order (BGRA2BGR).  The colour encodings
     * need colour input (trexhip_segment_color*); detection itself always works on cv::cvtColor(BGR2GRAY) (or color_channel). */
    int32_t pixel_encoding;
    /* Pre-processing options of RawProcessing::generate_binary that are NOT implemented (their arithmetic lives in the un-vendored
     * commons and nothing in the tree pins it).  They are part of the parameter block so that a caller can hand over what TRex's
     * settings say: any non-default value makes trexhip_create fail with TREXHIP_E_UNSUPPORTED -- never a silently different mask.
     *   image_adjust (+ image_contrast_increase / image_brightness_increase / image_square_brightness), blur_difference,
     *   equalize_histogram, correct_luminance      grabber/misc/default_config.cpp:121-129
     *   use_adaptive_threshold (+ adaptive_threshold_scale)                         core/default_config.cpp:1161-1162 */
    int32_t image_adjust, blur_difference, equalize_histogram, correct_luminance, use_adaptive_threshold;
    /* host tiles of a colour format with a gray / binary pixel_encoding (trexhip_segment_color): 0 (default) = the upload threads reduce
     * the tile to gray while they copy it into the pinned ring (a quarter / a third of the bytes cross PCIe; same fixed-point formula),
     * 1 = the colour tile is uploaded and reduced on the device.  The colour encodings always upload the colour tile. */
    int32_t device_color_reduce;
    int32_t reserved_[1];
} trexhip_params;
enum { TREXHIP_ENC_GRAY = 0, TREXHIP_ENC_R3G3B2 = 1, TREXHIP_ENC_RGB8 = 2 };   /* order of cmn::meta_encoding_t */

/* size class of a re-thresholded blob against track_size_filter (tracking/Tracker.cpp:864-912) */
#define TREXHIP_BLOB_IN_RANGE    0u   /* fish_size.in_range_of_one -> commit                     */
#define TREXHIP_BLOB_BELOW_RANGE 1u   /* recount < max_range().start -> filter_out(OutsideRange) */
#define TREXHIP_BLOB_BIG         2u   /* otherwise -> big_blob                                    */

/* HorizontalLine{y,x0,x1}, x1 inclusive (pv.cpp:509); 8 bytes */
typedef struct trexhip_run { uint16_t x0, x1, y, pad; } trexhip_run;

/* One blob = one blob::Pair (lines + pixels) plus the reductions the tracker asks of it
 * (pv::Blob::calculate_moments, Individual::weighted_centroid -- Individual.cpp:2414-2440).
 * Sums are exact integers so host-side float results do not depend on summation order. */
typedef struct trexhip_blob {
    uint32_t run_begin, n_runs;     /* index into the frame's run array (sorted by (y,x0))   */
    uint32_t pix_begin, n_pixels;   /* index into the frame's pixel array (gathered in run order) */
    uint16_t x0, y0, x1, y1;        /* inclusive bounding box                                */
    uint32_t bid;                   /* pv::bid of the blob (13/13/6-bit hash of first line)  */
    uint32_t px_min_max;            /* min | max << 8 of the grey values                     */
    uint32_t parent;                /* re-threshold results: pooled index of the detect blob; else 0xFFFFFFFF */
    uint32_t flags;                 /* re-threshold results: TREXHIP_BLOB_* size class; else 0 */
    uint64_t m10, m01;              /* sum x, sum y                                          */
    uint64_t m20, m11, m02;         /* sum x^2, sum x*y, sum y^2                             */
    uint64_t sp, spx, spy;          /* sum p, sum p*x, sum p*y                               */
} trexhip_blob;

typedef struct trexhip_frame_info {
    uint32_t n_blobs, n_runs, n_pixels;   /* kept (after size filter)                        */
    uint32_t blob_begin, run_begin, pix_begin; /* offsets of this frame in the pooled arrays */
    uint32_t n_raw_runs, n_raw_blobs;     /* before filtering                                */
    uint32_t flags;                       /* TREXHIP_FRAME_*                                 */
    uint32_t reserved[3];
} trexhip_frame_info;

/* Host view of one segmented batch (pooled arrays, pinned host memory owned by the ctx). */
typedef struct trexhip_batch_result {
    int32_t n_frames;
    uint32_t total_blobs, total_runs, total_pixels;
    const trexhip_frame_info* frames;   /* [n_frames]                                        */
    const trexhip_blob* blobs;          /* [total_blobs]; run_begin/pix_begin are FRAME-relative */
    const trexhip_run* runs;            /* [total_runs]                                      */
    const uint8_t* pixels;              /* [total_pixels * pixel_channels]                   */
    uint32_t pixel_channels;            /* bytes per pixel: 1 (gray, r3g3b2) or 3 (rgb8); pix_begin / n_pixels count PIXELS */
    uint32_t reserved_;
} trexhip_batch_result;

/* Device view of the same tables (for downstream device stages and torch interop). */
typedef struct trexhip_device_view {
    const trexhip_frame_info* frames;
    const trexhip_blob* blobs;
    const trexhip_run* runs;
    const uint8_t* pixels;
    const uint32_t* totals;             /* [3] total blobs, runs, pixels                     */
    const uint32_t* blob_frame;         /* [pool] frame index of each pooled blob            */
} trexhip_device_view;

typedef struct trexhip_ctx trexhip_ctx;

int trexhip_abi_version(void);
const char* trexhip_last_error(void);
void trexhip_default_params(trexhip_params* p, int32_t width, int32_t height);

/* BackgroundSubtraction::BackgroundSubtraction / Detection::init (python/Detection.cpp:16-58) */
int trexhip_create(const trexhip_params* p, trexhip_ctx** out);
/* BackgroundSubtraction::deinit (BackgroundSubtraction.cpp:118-120) */
void trexhip_destroy(trexhip_ctx* ctx);
/* The settings the reference re-reads on EVERY apply() (python/BackgroundSubtraction.cpp:137-143: cm_per_pixel, detect_size_filter;
 * RawProcessing reads its thresholds per call as well): trexhip_get_live_params copies the context's current values,
 * trexhip_update_params replaces them for every segment call that follows (the kernels take the settings by value at launch: this is a
 * host-side update, no device work; not to be called while another thread is inside a segment call of the same ctx).  Settings that size
 * or lay out buffers (frame size, capacities, pixel_encoding, morphology sizes) stay fixed for the life of the context.  More than 8
 * ranges or image_invert with a colour pixel_encoding are refused like in trexhip_create; the context keeps its previous values then. */
typedef struct trexhip_live_params {
    int32_t threshold, threshold_maximum, inclusive;                     /* as in trexhip_params */
    int32_t enable_difference, absolute_difference, image_invert, zero_is_background;
    int32_t n_ranges;                                                    /* detect_size_filter, 0 = accept all, at most 8 */
    double  cm_per_pixel;
    double  ranges[16];                                                  /* [start,end) pairs in cm^2 */
} trexhip_live_params;
int trexhip_get_live_params(trexhip_ctx* ctx, trexhip_live_params* out);
int trexhip_update_params(trexhip_ctx* ctx, const trexhip_live_params* lp);
/* use an external hipStream_t (e.g. torch's current stream); NULL = the ctx's own stream */
int trexhip_set_stream(trexhip_ctx* ctx, void* hip_stream);

/* BackgroundSubtraction::set_background -> Data::set (BackgroundSubtraction.cpp:86-101) */
int trexhip_set_background(trexhip_ctx* ctx, const uint8_t* gray, int32_t stride);
int trexhip_set_background_device(trexhip_ctx* ctx, const uint8_t* d_gray);
/* Background(image, meta_encoding_t::rgb8): a BGR / BGRA background.  Detection and the track-stage thresholds keep using its
 * cv::cvtColor(BGR2GRAY) (or the picked color_channel, as in trexhip_segment_color), which this call also installs as the gray
 * background; the colour image stays resident for the per-channel background-difference crops of the rgb8 pixel encoding
 * (imageFromLines' `differences`, Application/Tests/test_pixels.cpp:1381-1479). */
int trexhip_set_background_color(trexhip_ctx* ctx, const uint8_t* bgr, int32_t stride_bytes, int32_t channels, int32_t color_channel);
int trexhip_set_background_color_device(trexhip_ctx* ctx, const uint8_t* d_bgr, int32_t channels, int32_t color_channel);

/* background model from n sampled gray frames in HBM ("next" row of SURVEY.md 8f: Segmenter::trigger_average_generator,
 * ui/Segmenter.cpp:467-566; averaging_method grabber/misc/default_config.cpp:131): method 0 = mean (float accumulation in
 * sample order, rounded half-to-even), 1 = max, 2 = min, 3 = mode (most frequent value of the pixel, the smallest wins a tie; at most
 * 255 samples); the result becomes the context's background. */
int trexhip_generate_average_device(trexhip_ctx* ctx, const uint8_t* d_frames, int32_t n, int32_t method);
int trexhip_get_background(trexhip_ctx* ctx, uint8_t* gray, int32_t stride);

/* BackgroundSubtraction::apply(std::vector<TileImage>&&) hot loop (BackgroundSubtraction.cpp:146-316):
 * generate_binary + CPULabeling::run + size filter for n gray frames. */
int trexhip_segment_device(trexhip_ctx* ctx, const uint8_t* d_frames, int32_t n);
int trexhip_segment(trexhip_ctx* ctx, const uint8_t* const* frames, int32_t stride, int32_t n);
/* the same for the BGR / BGRA tile images TRex actually hands over (BackgroundSubtraction.cpp:162-180):
 * channels 3 or 4; color_channel < 0 (or >= channels) = cv::cvtColor(BGR2GRAY / BGRA2GRAY), else that channel */
int trexhip_segment_color(trexhip_ctx* ctx, const uint8_t* const* frames, int32_t stride, int32_t n,
                          int32_t channels, int32_t color_channel);
/* the same for n contiguous colour frames already in HBM ([n][height][width][channels]) */
int trexhip_segment_color_device(trexhip_ctx* ctx, const uint8_t* d_color_frames, int32_t n, int32_t channels, int32_t color_channel);
int trexhip_pixel_channels(trexhip_ctx* ctx);   /* bytes per pixel of the pixel arrays and channels of the crops: 1 or 3 (rgb8) */
/* device buffers for callers that do not link the HIP runtime themselves (the C++ adapters in trex_amd/host): plain
 * hipMalloc / hipFree / stream-ordered device-to-host and host-to-device copies (synchronous on return) on the context's device and stream */
int trexhip_device_alloc(trexhip_ctx* ctx, size_t bytes, void** out_device_ptr);
int trexhip_device_free(trexhip_ctx* ctx, void* device_ptr);
int trexhip_copy_to_host(trexhip_ctx* ctx, void* host_dst, const void* device_src, size_t bytes);
int trexhip_copy_to_device(trexhip_ctx* ctx, void* device_dst, const void* host_src, size_t bytes);
/* wait for the last segment call and copy its tables to pinned host memory.  Batches of up to 16 frames (TRex's default detect_batch_size is 1,
 * core/default_config.cpp:1113) leave the device as ONE kernel that writes the filled parts of all five tables into the pinned mirrors + one
 * stream synchronize; larger batches as two rounds of DMA copies (frame table and totals, then the tables at their exact sizes). */
int trexhip_fetch(trexhip_ctx* ctx, trexhip_batch_result* out);
/* trexhip_fetch in two halves, for a caller that needs the COUNTS on the host to go on (crops, posture and the identity table read the device
 * tables) and the blob / run / pixel tables only later (ABI 26).
 *   trexhip_fetch_begin  does what trexhip_fetch does until the frame table and the totals are on the host (the same checks, return codes and
 *                        messages), queues the copies of the three pooled tables on the context's stream, records an event behind them and
 *                        returns without waiting: `out` holds the counts and the pointers, out->frames is valid, the memory behind
 *                        out->blobs / runs / pixels is NOT until trexhip_fetch_wait has returned.  A batch of up to 16 frames and an empty batch
 *                        are served as by trexhip_fetch: nothing is pending afterwards.
 *   trexhip_fetch_wait   blocks until those copies have arrived; returns at once with nothing pending, so it may be called twice.
 * Every call that overwrites the device tables or the pinned mirrors (the segment calls, trexhip_load_frames_v6_device, trexhip_fetch[_begin],
 * trexhip_destroy) or reads the mirrors on the host (trexhip_posture_device, trexhip_posture_auto_device, trexhip_split_search_device) waits
 * first itself: a caller that forgets trexhip_fetch_wait gets the data of a plain fetch, never a race inside the library -- only its own reads of
 * out->blobs / runs / pixels are its own business.  trexhip_set_stream does not wait for pending copies: they stay on the stream they were
 * queued on (fetch_begin synchronised that stream in front of them), and work queued on the new stream is not ordered behind them.
 * (Two segment calls on the same frames give the same blobs but not the same pooled ORDER: a frame reserves its share of the pools when its
 * labelling ends.  The frame table's *_begin words are those of the segment call, whichever fetch reads them.) */
int trexhip_fetch_begin(trexhip_ctx* ctx, trexhip_batch_result* out);
int trexhip_fetch_wait(trexhip_ctx* ctx);
int trexhip_device_view_get(trexhip_ctx* ctx, trexhip_device_view* out);
int trexhip_synchronize(trexhip_ctx* ctx);

/* ---- .pv frame bodies ------------------------------------------------------------------------------
 * pv::Frame::serialize (ProcessedVideo/pv.cpp:666-703) for every frame of the last fetched batch, on the device, in the layout
 * pv::Frame::read_from accepts for file version V_6 (pv.cpp:296-420) -- the newest one whose line type is in the reference tree
 * (LegacyShortHorizontalLine, pv.h:17-52; >= V_7 use commons' ShortHorizontalLine): u8 compression_flag = 0, u64 timestamp, u16 n,
 * n x {u16 start_y, u16 mask_size, mask_size x {u16 x0, u16 x1 << 1 | eol}, 1 byte per pixel}.  Gray pixel arrays, width <= 32768.
 *   timestamps  host array [n_frames] (relative to the file header's timestamp) or NULL (zeros)
 *   d_out       the bodies back to back, in frame order;  d_offsets [n_frames + 1] byte offsets (d_offsets[n_frames] = total bytes;
 *               when that exceeds `capacity` nothing valid was written: call again with a larger buffer)
 * Compression and the index table: trexhip_pv_write_frames below (host side); the file header (pv.cpp:842-990) is not produced. */
int trexhip_pack_frames_v6_device(trexhip_ctx* ctx, const uint64_t* timestamps, uint8_t* d_out, size_t capacity, uint64_t* d_offsets);

/* The inverse: pv::Frame::read_from (ProcessedVideo/pv.cpp:296-420, version V_6: u64 timestamp :347-351, LegacyShortHorizontalLine
 * masks :377-388, pixels :399-403) for a batch of stored frames, on the device.  Tracking runs on frames read back from the file
 * (Tracker::prefilter, posture, FilterCache, SplitBlob, the identity network): behind this call and trexhip_fetch the context holds the
 * tables it would hold behind trexhip_segment_device and trexhip_fetch on the frames the file was converted from, and every track-stage
 * call (re-threshold, split search, posture, midline, crops, id table) runs on them unchanged.
 *   d_bodies / d_offsets   what trexhip_pack_frames_v6_device writes (or trexhip_pv_read_frames returns, uploaded): uncompressed bodies
 *                          back to back, each starting with its flag byte 0; d_offsets [n_frames + 1].  1 <= n_frames <= max_batch
 *   d_timestamps           device [n_frames] or NULL: receives every frame's timestamp
 * Frames are pooled in frame order, blobs keep file order, every field of trexhip_blob is what the detect stage computes for the same
 * blob.  The grey values the track stage reads come from a frame image owned by the context into which the call paints every blob's
 * stored pixels; they are final (the segmenter stored 255 - p under image_invert), so the batch is not inverted again downstream.
 * A frame beyond max_blobs / max_runs / max_pixels gets the overflow flags of a segmented frame; a frame whose bytes break the layout
 * (the rules: trex_amd/csrc/pv_read.h; no read passes d_offsets[f + 1] whatever the bytes say) gets TREXHIP_FRAME_MALFORMED, keeps no
 * blob, and trexhip_fetch returns TREXHIP_E_INVALID ("malformed") for the batch; the other frames are unaffected either way.
 * Gray pixel arrays, width <= 32768, max_blobs <= 65535 (TREXHIP_E_UNSUPPORTED otherwise, as the packer).  Only enqueues work on the
 * context's stream: no host synchronisation. */
int trexhip_load_frames_v6_device(trexhip_ctx* ctx, const uint8_t* d_bodies, const uint64_t* d_offsets, int32_t n_frames, uint64_t* d_timestamps);

/* ---- .pv data section: per-frame LZO1X compression + index table (host side, no GPU needed) -------
 * trexhip_pv_write_frames = the tail of pv::Frame::serialize (pv.cpp:705-772: a pack of >= 15000 bytes -- every pack when
 * always_compress, which is what the rgb8 encoding does -- goes through LZO1X-1 and is kept compressed if 8 + compressed < uncompressed)
 * + pv::File::add_individual (pv.cpp:1488-1496: u8 compression_flag, then either the pack or u32 compressed size, u32 uncompressed size,
 * compressed bytes; the frame's offset in the file goes to the index table) for the frames of trexhip_pack_frames_v6_device copied to
 * the host (`bodies` + `offsets`, each starting with its compression_flag 0).
 *   file_offset  where `out` will sit in the file (the data section starts right behind the header, pv.cpp:1079-1095)
 *   out          capacity >= sum of the bodies is always enough;  *out_bytes = bytes written
 *   index_table  [n_frames] u64 file offsets = what pv::Header::update writes as the index table (pv.cpp:1181-1192) and
 *                Header::read loads (pv.cpp:986-990)
 * The stream is read back by pv::Frame::read_from's lzo1x_decompress (pv.cpp:316-340).  The compressor is this library's own LZO1X
 * encoder, not a byte-for-byte lzo1x_1_compress (ProcessedVideo/lzo/minilzo.c): a reader only ever sees the decompressed pack.
 * Still blocked on the un-vendored commons: the header's strings / cv::Size encoding (DataFormat) and the >= V_7 line type. */
size_t trexhip_lzo1x_bound(size_t n);            /* pv.cpp:712 OUT_LEN: n + n / 16 + 64 + 3 */
int trexhip_lzo1x_compress(const uint8_t* in, size_t n, uint8_t* out, size_t capacity, size_t* out_len);
int trexhip_pv_write_frames(const uint8_t* bodies, const uint64_t* offsets, int32_t n_frames, int32_t always_compress, uint64_t file_offset,
                            uint8_t* out, size_t capacity, uint64_t* index_table, size_t* out_bytes);
/* Reading it back.  trexhip_lzo1x_decompress = lzo1x_decompress as pv::Frame::read_from calls it (pv.cpp:326-333; decoder
 * ProcessedVideo/lzo/minilzo.c): this library's own decoder, which checks both buffers on every copy -- a truncated or overlong stream,
 * or an output beyond `capacity`, is TREXHIP_E_INVALID, never an access outside either buffer.
 * trexhip_pv_read_frames = the head of pv::Frame::read_from (pv.cpp:313-340) for n_frames frames of a data section: frame f starts at
 * data[index_table[f] - file_offset]; flag 0: the pack is copied (its extent is the chain of its blob sizes, bounded by `bytes`);
 * flag 1: u32 compressed size, u32 uncompressed size, the stream is decompressed and given a leading flag byte 0.  bodies / offsets
 * [n_frames + 1] are then what trexhip_load_frames_v6_device takes.  Everything is bounded by `bytes` and `capacity`
 * (TREXHIP_E_INVALID beyond either; *out_bytes = bytes written).  bodies == NULL asks for the sizes only: offsets and *out_bytes are
 * filled, nothing is decompressed. */
int trexhip_lzo1x_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t capacity, size_t* out_len);
int trexhip_pv_read_frames(const uint8_t* data, size_t bytes, uint64_t file_offset, const uint64_t* index_table, int32_t n_frames,
                           uint8_t* bodies, size_t capacity, uint64_t* offsets, size_t* out_bytes);

/* ---- track-stage re-threshold -----------------------------------------------------------------
 * Tracker::prefilter's arithmetic (tracking/Tracker.cpp:765-849): for every kept blob of the last segmented
 * batch, pixel::threshold_blob(blob, threshold, background) -- keep a pixel iff diff >= threshold with
 * method 0 = |bg-p| (track_threshold_is_absolute), 1 = max(bg-p,0) (signed), 2 = p (no background
 * subtraction); runs split where pixels fail, survivors re-labelled into sub-blobs.  Nothing is dropped:
 * each sub-blob carries `parent` (pooled index of its detect blob) and `flags` (TREXHIP_BLOB_* class
 * against size_ranges = track_size_filter, cm^2), so the host applies prefilter's remaining policy
 * (recount = sum of n_pixels over a parent's sub-blobs).  Results are a second table set. */
int trexhip_rethreshold_device(trexhip_ctx* ctx, int32_t threshold, int32_t method, const double* size_ranges, int32_t n_ranges);
/* the same with one threshold per detect blob (device array indexed by pooled blob index; negative = skip the blob):
 * the building block of SplitBlob::apply_threshold (tracking/SplitBlob.cpp:130-164), which tries different thresholds on
 * different merged blobs; the search over thresholds stays with the caller */
int trexhip_rethreshold_per_blob_device(trexhip_ctx* ctx, int32_t threshold, const int32_t* d_blob_thresholds, int32_t method,
                                        const double* size_ranges, int32_t n_ranges);
int trexhip_fetch_rethreshold(trexhip_ctx* ctx, trexhip_batch_result* out);

/* ---- Tracker::prefilter's blob policy ---------------------------------------------------------------------
 * The decisions of Tracker::prefilter (tracking/Tracker.cpp:742-914) for every frame of the last fetched batch (segmented or loaded), on
 * the device: the call runs the re-threshold of trexhip_rethreshold_device at track_threshold (the same code path; the context's second
 * table set holds its result afterwards and trexhip_fetch_rethreshold / posture table 1 read it as usual) and then walks the reference's
 * loop (:806-914) per detect blob:
 *   1. check_blob(own, false): rect_overlaps_shapes(bounds, track_include) and track_ignore_bdx (:786-801);
 *   2. the gate of :828-831 -- no track_size_filter or close_to_minimum_of_one(recount, 0.5), and track_threshold > 0 -- decides whether
 *      the blob's sub-blobs stand for it;
 *   3. each sub-blob through check_precise_not_ignored on its centre: track_ignore, track_include, bdx of itself or its parent (:742-763);
 *   4. the un-thresholded blob instead when the gate was closed or nothing survived the threshold (:853-858), through the same check;
 *   5. per surviving entry in_range_of_one(recount) -> the second-threshold test (:865-874) -> committed; else OutsideRange below
 *      max_range().start; else big.
 * cm_per_pixel is the context's live value.  Ordered on the context's stream, no host synchronisation.
 * Entries, with cap = max_batch * max_blobs: e = f * max_blobs + k is sub-blob k of frame f of the second table set (pooled index
 * frames[f].blob_begin + k of trexhip_fetch_rethreshold), e = cap + f * max_blobs + k is detect blob k of frame f (pooled index
 * frames[f].blob_begin + k of trexhip_fetch) standing un-thresholded or filtered by step 1.  Entries are numbered by frame and not by
 * pooled index because both table sets pool their frames in the order the frames finish, which differs from call to call: numbered this
 * way d_decision, d_order and d_counts (and d_second_count) of two calls on the same frames are the same bytes, whether the batch was
 * segmented or loaded.
 *   d_decision   [2 * cap] bytes, one per entry: TREXHIP_DECISION_COMMITTED, TREXHIP_DECISION_BIG, TREXHIP_DECISION_FILTERED + reason,
 *                or TREXHIP_DECISION_NONE (not an entry: beyond the tables, a sub-blob whose parent stands for itself or was filtered,
 *                a detect blob whose sub-blobs stand for it)
 *   d_order      [n_frames][2 * max_blobs] int32: per frame the committed entries, then the big entries, each in the order the reference's
 *                loop appends them (detect blob order, table order of the sub-blobs inside one detect blob); -1 behind them
 *   d_counts     [n_frames][4] int32: committed, big, filtered out, and 1 when the frame decided nothing
 *   d_presumed_nr[total detect blobs] int32, by POOLED index of the detect table: 2 for the detect blob a big entry belongs to
 *                (split_expectation(2, false), PrefilterBlobs.cpp:223), else 0: what trexhip_split_search_device takes
 * A frame flagged overflow or malformed (in either table set) keeps its flags, decides nothing (d_counts[f][3] = 1, its decision bytes
 * stay TREXHIP_DECISION_NONE) and leaves the other frames alone.
 * Refused: more than 8 size ranges, more than 64 shapes or 4096 points in a list (TREXHIP_E_UNSUPPORTED); thresholds outside 0..255, a
 * batch that was not fetched (TREXHIP_E_INVALID); a frame whose detect blobs together with the shape tables exceed the 160 KB of LDS of
 * one workgroup -- about 9000 blobs in a frame with full shape tables, 13000 without -- (TREXHIP_E_CAPACITY).
 * Not on this path: tags, instance segmentations, categories, classes and prediction confidence (Tracker.cpp:776-784, :876-904) belong
 * to the YOLO / categorisation backends; there is no field for them.
 * UNPINNED (the reference calls into the un-vendored commons; each is implemented from its documented meaning):
 *   pnpoly                   W. R. Franklin's crossing test in float, edges (j, i) with j = i - 1 cyclic
 *   Bounds::contains         x <= px < x + width and y <= py < y + height
 *   Bounds::overlaps         open intersection: a.x < b.x + b.width, b.x < a.x + a.width, and the same in y
 *   Bounds::insert_point     x, y = minimum, width, height = maximum; PrefilterBlobs.cpp:364 starts the polygon's box at
 *                            (0, 0, FLT_MAX, FLT_MAX), so as written it reaches from min(0, points) to FLT_MAX: kept as written
 *   Blob::bounds / center    pos = (x0, y0), size = (x1 - x0 + 1, y1 - y0 + 1), center = pos + size * 0.5
 *   recount                  surviving pixels * cm^2 in float (as trexhip_rethreshold_device); force_set_recount(threshold) at :771 =
 *                            all pixels of the blob * cm^2 without a pixel pass
 *   Range<float>::contains   [start, end), as Range<double> in the size filters
 *   pv::FilterReason         its numbering is not in the tree: TREXHIP_FILTER_* below is this library's own */
enum { TREXHIP_FILTER_OUTSIDE_INCLUDE = 0, TREXHIP_FILTER_INSIDE_IGNORE = 1, TREXHIP_FILTER_BDX_IGNORED = 2, TREXHIP_FILTER_OUTSIDE_RANGE = 3,
       TREXHIP_FILTER_SECOND_THRESHOLD = 4 };
enum { TREXHIP_DECISION_COMMITTED = 0, TREXHIP_DECISION_BIG = 1, TREXHIP_DECISION_FILTERED = 16, TREXHIP_DECISION_NONE = 255 };
typedef struct trexhip_prefilter_params {
    int32_t track_threshold;            /* core/default_config.cpp:937; 0 = nothing is thresholded (:830)                          */
    int32_t method;                     /* difference, as trexhip_rethreshold_device: 0 |bg - p|, 1 max(bg - p, 0), 2 p            */
    int32_t track_threshold_2;          /* :939; 0 = off                                                                          */
    int32_t n_ranges;                   /* track_size_filter, at most 8 ranges                                                    */
    float   threshold_ratio_range[2];   /* :938 (0.5, 1.0)                                                                        */
    double  size_ranges[16];            /* [start, end) pairs in cm^2                                                             */
} trexhip_prefilter_params;
/* track_include / track_ignore: device float2 points of all shapes back to back and device offsets [n_shapes + 1] into them; a shape of
 * 2 points is a rectangle (corner, opposite corner), of more than 2 a polygon, of fewer nothing (PrefilterBlobs.cpp:328-385).
 * track_ignore_bdx: per frame of the batch a sorted list of pv::bid words, d_ignore_bdx_offsets [n_frames + 1]; NULL = none.
 * d_second_count: optional OUTPUT, device [2 * cap] int32 indexed like d_decision: the pixels at track_threshold_2 of every entry that
 * reached the size test in range, -1 elsewhere (and everywhere with track_threshold_2 == 0). */
typedef struct trexhip_prefilter_tables {
    const float*    d_include_points;  const int32_t* d_include_offsets;  int32_t n_include_shapes, n_include_points;
    const float*    d_ignore_points;   const int32_t* d_ignore_offsets;   int32_t n_ignore_shapes, n_ignore_points;
    const uint32_t* d_ignore_bdx;      const int32_t* d_ignore_bdx_offsets;  int32_t n_ignore_bdx, reserved_;
    int32_t*        d_second_count;
} trexhip_prefilter_tables;
void trexhip_default_prefilter_params(trexhip_prefilter_params* p);
int trexhip_prefilter_device(trexhip_ctx* ctx, const trexhip_prefilter_params* pp, const trexhip_prefilter_tables* tables /* NULL = none */,
                             uint8_t* d_decision, int32_t* d_order, int32_t* d_counts, int32_t* d_presumed_nr);

/* ---- splitting merged blobs: SplitBlob's threshold search -----------------------------------------------
 * SplitBlob::split (tracking/SplitBlob.cpp:419-800) for blob_split_algorithm threshold / threshold_approximate: for every detect blob
 * of the last batch with presumed_nr[blob] > 0 (PrefilterBlobs::split_big's split_expectation::number, PrefilterBlobs.cpp:217-236;
 * <= 0 = not a candidate) find the smallest threshold at which pixel::threshold_blob on the blob's difference values
 * (apply_threshold :130-179) is accepted by evaluate_result_multiple (:193-255).  The reference re-labels the blob on the CPU for
 * every tried threshold; here one wave per blob keeps the difference values in LDS.  Large blobs, which the reference searches
 * with 4 pool threads (:735-760), get the deterministic sequential result (identical for `threshold`, see oracle/trex_split.c).
 *   d_thresholds [n_blobs] int32: the threshold to hand to trexhip_rethreshold_per_blob_device (which then yields the sub-blobs
 *                                 threshold_blob returns), or -1 when the blob cannot be split / is no candidate
 *   d_info       [n_blobs]: what the search saw.  Of the sub-blobs, those with n_pixels * cm^2 < min_size_bound are not part
 *                           of SplitBlob::split's result (:204-221); the rest is returned sorted by (num_pixels, blob_id) descending
 *                           and shifted by -bounds().pos() (:166-172), which the caller does on the fetched table.
 * Needs a fetched batch (n_blobs = total_blobs).  Three size classes by LDS need (2048 / 16384 / 61440 pixels per blob); blobs with
 * more than 61440 pixels or 2048 lines (or, at a threshold the search reaches, more lines after thresholding than their class holds:
 * 1024 / 2048 / 4096) report status 2 and no threshold.
 * cm_per_pixel: the sizes compared here are (float)n_pixels * sqcm with sqcm = (float)(cm_per_pixel * cm_per_pixel) of the context's
 * double.  The reference holds cm_per_pixel as a float and squares it in float; for values such as 0.37, 0.1 or 0.0173 the two differ
 * by one ulp unless the double handed to the context is itself a widened float ((double)(float)cm), and then a blob whose size lies on
 * the edge of a size range is decided differently.  Pass a widened float where the reference's decisions have to be met exactly. */
typedef struct trexhip_split_params {
    int32_t track_threshold;                 /* core/default_config.cpp track_threshold            */
    int32_t track_posture_threshold;
    int32_t calculate_posture;               /* initial threshold = (calculate_posture ? max(both) : track_threshold) + 1 (:512) */
    int32_t algorithm;                       /* blob_split_algorithm: 0 none, 1 threshold (default, :923), 2 threshold_approximate; 3 fill (cv::watershed, :419-485) and 4 fill_approximate are refused with TREXHIP_E_UNSUPPORTED */
    float   blob_split_max_shrink;           /* :921 (0.2) */
    float   blob_split_global_shrink_limit;  /* :922 (0.2) */
    int32_t n_ranges;                        /* track_size_filter, cm^2, at most 8 ranges */
    int32_t reserved_;
    double  size_ranges[16];
} trexhip_split_params;
typedef struct trexhip_split_info {
    int32_t threshold;                       /* best_match.threshold as the reference records it, or -1 */
    int32_t effective_threshold;             /* the threshold apply_threshold really used for it (clamped to the blob's smallest difference) */
    int32_t status;                          /* 0 searched, 2 capacity, 3 not a candidate / frame overflowed */
    int32_t initial_action;                  /* split::Action of the first try: 1 KEEP_ABORT, 2 REMOVE, 3 ABORT, 4 TOO_FEW, 5 SKIP */
    int32_t n_result;                        /* blobs SplitBlob::split returns */
    int32_t n_evaluated;                     /* labelling passes spent on the blob */
    int32_t min_pixel, max_pixel;            /* range of the difference values (:142-156) */
    float   first_size;                      /* size of the biggest sub-blob at the first try, cm^2 (:530-531) */
    float   reserved_;
    double  min_size_bound;
} trexhip_split_info;
void trexhip_default_split_params(trexhip_split_params* p);
int trexhip_split_search_device(trexhip_ctx* ctx, const trexhip_split_params* sp, int32_t method, const int32_t* d_presumed_nr,
                                int32_t n_blobs, int32_t* d_thresholds, trexhip_split_info* d_info);

/* ---- posture (outline -> midline) -----------------------------------------------------------------
 * posture::calculate_posture (tracking/Posture.cpp:305-399) for every blob of a table of the last batch
 * (table 0 = detect blobs, 1 = re-thresholded sub-blobs, i.e. the caller picks track_posture_threshold through
 * trexhip_rethreshold_device).  One pass per call: the reference's retry loop "threshold += 2 until a midline is found"
 * (:331-381) only ever re-runs blobs too small for a midline and ends in its first-outline fallback, which is what one pass
 * returns for them (status 3 / 4 with the outline) -- shown on the CPU restatement, tests/test_posture_oracle.py.
 * Outputs (caller-owned device memory, pooled order like trexhip_fetch):
 *   outline  [n_blobs][max_points] float2   resampled, smoothed, EFT-approximated outline rotated so that point 0 is
 *                                           the tail (what Outline holds after calculate_midline), relative to the
 *                                           blob's bounds().pos()
 *   segments [n_blobs][max_points/2+1] float4 = MidlineSegment{pos.x, pos.y, height, l_length} (Outline.h:241-250)
 *   info     [n_blobs] status 0 ok / 1 empty / 2 capacity (more than max_points traced outline points, 2048 lines or 1022 rows) /
 *                      3 no curvature peak / 4 too few midline segments */
typedef struct trexhip_posture_params {
    float   outline_resample;               /* core/default_config.cpp:898  (1)    */
    int32_t outline_smooth_samples;         /* :890 (4)                            */
    int32_t outline_smooth_step;            /* :889 (1)                            */
    int32_t outline_approximate;            /* :888 (3)                            */
    float   outline_curvature_range_ratio;  /* :891 (0.03)                         */
    float   midline_walk_offset;            /* :892 (0.025)                        */
    int32_t max_points;                     /* capacity per blob (outline points; the traced lattice outline has 2 per pixel edge), even, 8..4096 */
    /* not implemented, refused with TREXHIP_E_UNSUPPORTED when switched on (never silently ignored):
     *   posture_closing_steps > 0 (Posture.cpp:335, morphological closing inside threshold_get_biggest_blob),
     *   peak_mode = broad (1; Outline.cpp:627-661; 0 = pointy, the default :897),
     * posture_direction_smoothing is not used by the posture call: the window is the tracker's (Individual::calculate_previous_vector);
     * with a value > 1 the reference hands the resulting movement direction to Midline::post_process -- trexhip_midline_movement_device */
    int32_t posture_closing_steps, peak_mode, posture_direction_smoothing;
} trexhip_posture_params;
typedef struct trexhip_posture_info { int32_t status, n_outline, n_segments, tail_index, head_index, n_traced, reserved[2]; } trexhip_posture_info;
void trexhip_default_posture_params(trexhip_posture_params* p);
int trexhip_posture_device(trexhip_ctx* ctx, int32_t table, const trexhip_posture_params* pp, int32_t n_blobs,
                           float* d_outline, float* d_segments, trexhip_posture_info* d_info);

/* posture::calculate_posture WITH its retry loop (Posture.cpp:305-399), for every DETECT blob of the last fetched batch: threshold =
 * track_posture_threshold; repeat { biggest sub-blob at that threshold (pixel::threshold_get_biggest_blob; method as in
 * trexhip_rethreshold_device) -> outline relative to the original blob -> midline; done on success; else threshold += 2 } until the
 * sub-blob has fewer than max(1, pixels / 10) pixels or threshold >= track_posture_threshold + 100; without success the first outline
 * that could be traced is returned without a midline (status of the last attempt, n_segments 0).  Outputs as trexhip_posture_device
 * (pooled order of the detect table); d_threshold_used / d_iterations ([n_blobs] int32, may be NULL) = the threshold whose result is
 * returned (-1: none) and the attempts made.  Uses (overwrites) the context's re-threshold tables. */
int trexhip_posture_auto_device(trexhip_ctx* ctx, const trexhip_posture_params* pp, int32_t method, int32_t track_posture_threshold,
                                int32_t n_blobs, float* d_outline, float* d_segments, trexhip_posture_info* d_info,
                                int32_t* d_threshold_used, int32_t* d_iterations);

/* Midline::post_process (no movement information, posture_direction_smoothing <= 1; Outline.cpp:895-1060) followed by
 * Midline::normalize() (Outline.cpp:1270-1454; call site Individual.cpp:1369-1372) for every blob of a posture call.
 *   d_segments: the segments buffer of trexhip_posture_device (same max_points); post-processed IN PLACE (head part straightened)
 *   d_midline : [n_blobs][midline_resolution] float4 = MidlineSegment{pos.x,pos.y,height,l_length}, head at the origin
 *   info      : status 0 ok / 1 no midline / 2 resampling did not yield midline_resolution points (normalize() == nullptr);
 *               len, angle, offset = Midline::len() / angle() / offset() (blob-local coordinates, like the outline) */
typedef struct trexhip_midline_params {
    int32_t midline_resolution;             /* core/default_config.cpp:894 (25)   */
    float   midline_stiff_percentage;       /* :893 (0.15)                        */
    int32_t midline_invert;                 /* :901 (false)                       */
    int32_t midline_start_with_head;        /* :900 (false)                       */
} trexhip_midline_params;
typedef struct trexhip_midline_info { int32_t status, n; float len, angle, offx, offy; int32_t reserved[2]; } trexhip_midline_info;
void trexhip_default_midline_params(trexhip_midline_params* p);
int trexhip_midline_device(trexhip_ctx* ctx, const trexhip_midline_params* mp, int32_t n_blobs, int32_t max_points,
                           const trexhip_posture_info* d_posture_info, float* d_segments, float* d_midline,
                           trexhip_midline_info* d_midline_info);
/* The same with MovementInformation::direction per blob (posture_direction_smoothing > 1: Individual.cpp:1364-1369 hands
 * calculate_previous_vector(frame) to post_process): d_movement_direction [n_blobs][2] float (x, y), (0, 0) = no information for that
 * blob; NULL = trexhip_midline_device.  A midline whose direction (Midline::midline_direction, Outline.cpp:870-887) points against the
 * movement -- acos(-direction . movement) < acos(direction . movement), :937 -- is turned round; trexhip_midline_info.reserved[0] = 1 for
 * such a blob (`_inverted_because_previous`): the caller swaps its head and tail index (:959).  The vector itself is tracker state (the
 * previous frames' velocities): the caller computes it. */
int trexhip_midline_movement_device(trexhip_ctx* ctx, const trexhip_midline_params* mp, int32_t n_blobs, int32_t max_points,
                                    const trexhip_posture_info* d_posture_info, float* d_segments, float* d_midline,
                                    trexhip_midline_info* d_midline_info, const float* d_movement_direction);

/* ---- crops ------------------------------------------------------------------------------------
 * constraints::diff_image (tracking/FilterCache.cpp:265-294): one out_w x out_h uint8 crop per blob of the
 * last segmented batch, pooled order (blob i of trexhip_fetch == crop i).  n_blobs = total_blobs of that
 * batch ([n][out_h][out_w][3] for the rgb8 pixel encoding, colour codes warped with nearest neighbour for r3g3b2; the difference modes of rgb8 are per-channel
 * differences against the colour background of trexhip_set_background_color, r3g3b2 crops hold raw codes only).  normalization: individual_image_normalization none or
 * moments (posture / legacy: next function).  difference: 0 = grey
 * values, 1 = |bg - p|, 2 = max(bg - p, 0)  (track_background_subtraction, FilterCache.cpp:171-175).
 * Sizes: any out_w, out_h > 0, square or not.  trexhip_crops_device (none AND moments) needs out_w * out_h * channels to be a multiple of
 * 16 bytes (the un-normalised gather clears its crop with 16-byte stores; the crop buffer 16-byte aligned): TREXHIP_E_INVALID otherwise
 * (TREXHIP_E_UNSUPPORTED for rgb8).  trexhip_crops_transformed_device and trexhip_crops_posture_device write single bytes and take any size,
 * e.g. 50 x 50.  Output rows / columns beyond 256 compute their fixed-point terms per pixel instead of from a table: same result.
 * Blobs: no limit on size.  The warp keeps a blob's lines in LDS up to 2048 lines and 1024 rows and paints bounding boxes of up to
 * 16384 bytes (pixels x channels) into LDS; larger blobs read their lines from global memory (a bisection per tap: slow, bit-identical). */
enum { TREXHIP_NORMALIZE_NONE = 0, TREXHIP_NORMALIZE_MOMENTS = 1, TREXHIP_NORMALIZE_POSTURE = 2 };
int trexhip_crops_device(trexhip_ctx* ctx, uint8_t* d_crops, int32_t n_blobs, int32_t out_w, int32_t out_h,
                         int32_t normalization, int32_t difference);

/* posture / legacy normalisation (FilterCache.cpp:267-274): the caller supplies, per blob in pooled order, the 2x3 row-major
 * float matrix of Midline::transform(normalize).toCV() (Outline.cpp:1237-1255) and the (median) midline length; the library
 * applies normalize_image (FilterCache.cpp:21-115): translate(size/2) . scale(individual_image_scale) .
 * translate(len*0.4 | legacy: (-len/2, 0)) . tr, then cv::warpAffine INTER_LINEAR in OpenCV's 8-bit fixed point. */
int trexhip_crops_transformed_device(trexhip_ctx* ctx, uint8_t* d_crops, int32_t n_blobs, int32_t out_w, int32_t out_h,
                                     const float* transforms, const float* midline_lengths, int32_t use_legacy,
                                     float image_scale, int32_t difference);
/* the same with tr = Midline::transform(posture | legacy) built from trexhip_midline_device's info (device pointer, pooled
 * order; blobs without a midline get an all-zero crop: diff_image returns nullptr for them, FilterCache.cpp:268-270).
 * midline_lengths: host array, the individuals' median midline length per blob (FilterCache.cpp:272), or NULL to use
 * each blob's own Midline::len(). */
int trexhip_crops_posture_device(trexhip_ctx* ctx, uint8_t* d_crops, int32_t n_blobs, int32_t out_w, int32_t out_h,
                                 const trexhip_midline_info* d_midline_info, const float* midline_lengths, int32_t use_legacy,
                                 float image_scale, int32_t difference);

/* ---- identity network (V118_3) -------------------------------------------------------------
 * VINetwork::load_weights (ml/VisualIdentification.cpp) / visual_recognition_torch.py:841-921: takes the
 * flat fp32 blob described in trex_amd/weights.py (state_dict order; tools/convert_weights.py makes it
 * from a TRex <base>_dict.pth).  BatchNorm is folded and the tensors repacked on load.  The blob's header carries the network's
 * individual_image_size W x H: any 8 <= W, H <= 256 (square or not; TREXHIP_E_UNSUPPORTED outside), crops are then [n][H][W][C].
 * 80 x 80 runs the tuned chain, every other size a generic one (conv1 exact fp32, conv2 / conv3 in the precision mode below, fc1 exact
 * fp32).  trexhip_crops_device needs W * H * C to be a multiple of 16 bytes (the posture / transformed crop calls do not, see "crops");
 * other sizes (e.g. 50 x 50 gray, un-normalised) take crops made on the host through trexhip_identify.  Loading another size on the same context replaces the network. */
int trexhip_load_weights(trexhip_ctx* ctx, const void* blob, size_t bytes);
int trexhip_num_classes(trexhip_ctx* ctx);
int trexhip_network_channels(trexhip_ctx* ctx);   /* channels of the crops the loaded network expects (1 or 3); 0 without weights */
/* the crop size W x H the loaded network expects; 0 x 0 without weights.  Either pointer may be NULL. */
int trexhip_network_image_size(trexhip_ctx* ctx, int32_t* width, int32_t* height);
/* The architecture of the network: TRex's setting visual_identification_version (core/default_config.h:83), a checkpoint's
 * metadata.model_type.  The blob's header word 6 carries it (0 in every blob written before ABI 17, which keep their meaning):
 *   TREXHIP_NET_V118_3  visual_identification_network_torch.py:184-258, sizes 8..256 each way -- the chains above
 *   TREXHIP_NET_V100    :328-382   8..256      TREXHIP_NET_V110  :262-324   8..256
 *   TREXHIP_NET_V119    :106-180   16..256     TREXHIP_NET_V200  :30-102    27..256
 * The four others run one generic chain (cnn_arch.hip): first layer exact fp32, the further convolutions in the precision mode below with the
 * same range guard, fc1 exact fp32; a call's crops are walked in chunks of trexhip_identify_chunk_crops (a constant of version and size), and a
 * crop's row does not depend on its chunk.  A smaller size is TREXHIP_E_UNSUPPORTED, an id outside 0..4 TREXHIP_E_INVALID.  V118_3, v100 and v110
 * train (trexhip_trainer_create, ABI 18); a trainer refuses v119 and v200 with TREXHIP_E_UNSUPPORTED.  (ABI 17) */
enum { TREXHIP_NET_V118_3 = 0, TREXHIP_NET_V100 = 1, TREXHIP_NET_V110 = 2, TREXHIP_NET_V119 = 3, TREXHIP_NET_V200 = 4 };
/* the loaded network's TREXHIP_NET_*; 0 without a context or weights, like trexhip_num_classes (VINetwork's
 * visual_identification_version, ml/VisualIdentification.cpp) */
int trexhip_network_version(trexhip_ctx* ctx);
/* bytes of the blob trexhip_load_weights takes for that version (trex_amd/weights.py shapes(arch=...)); 0 for a version, channel count or
 * size that no network has.  No reference counterpart (a state_dict knows its own size). */
size_t trexhip_network_blob_bytes(int32_t version, int32_t classes, int32_t channels, int32_t width, int32_t height);
/* crops per chunk of an identify call on the loaded network; *crops = 0 for V118_3, where a call is not chunked, and without weights.
 * No reference counterpart (predict_numpy walks batches of its own choosing, visual_recognition_torch.py:290-352). */
int trexhip_identify_chunk_crops(trexhip_ctx* ctx, int32_t* crops);
/* arithmetic of conv1..fc1.  All modes but BF16X3 meet the 1e-4 softmax bar against the fp32 reference network:
 *   TREXHIP_CNN_FP16X3 (default): every fp32 operand as two fp16 pieces (22 mantissa bits), 3 piece products per product on the
 *       fp16 matrix cores, fp32 accumulate; an activation outside the fp16 range raises a device flag and the layer stack is
 *       re-run by the BF16X6 kernels (never a silent wrong answer);
 *   TREXHIP_CNN_BF16X6: three bf16 pieces, 6 piece products;  TREXHIP_CNN_FP32: exact fp32 MFMA (v_mfma_f32_32x32x2_f32);
 *   TREXHIP_CNN_BF16X3: three piece products only (~2^-16 relative per product) -- for experiments. */
enum { TREXHIP_CNN_FP32 = 0, TREXHIP_CNN_BF16X6 = 1, TREXHIP_CNN_BF16X3 = 2, TREXHIP_CNN_FP16X3 = 3 };
int trexhip_set_identity_precision(trexhip_ctx* ctx, int32_t mode);
/* VINetwork::probabilities (ml/VisualIdentification.cpp:440-458) -> predict_numpy
 * (visual_recognition_torch.py:290-352): crops are uint8 NHWC [n][H][W][C] of the loaded network (trexhip_network_image_size,
 * trexhip_network_channels; values 0..255, no scaling), probs is [n][classes] float32 softmax rows.  d_logits may be NULL. */
int trexhip_identify_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n, float* d_probs, float* d_logits);
/* The part of the next trexhip_identify_device(ctx, d_crops, n, ...) that needs nothing but the crops' bytes and the loaded network, queued
 * now on the context's stream: which passes, row pairs and fc1 rows the crops' blobs reach, and the background rows of the others (k_crop_bands
 * ... k_v3_fill and k_act3_fill).  For a caller that drives two contexts and lets only one network run at a time: issue this BEFORE
 * waiting for the other context's network, so that these small latency-bound kernels run beside its tail and not behind it.  No reference
 * counterpart (predict_numpy is one call).
 *   - The next trexhip_identify_device on the context takes the record this call leaves, whatever its arguments: it skips those launches if
 *     crops pointer, n, precision mode, stream and the loaded weights / batch buffers are the ones prepared for, and runs the whole chain as ever
 *     otherwise.  Its results are bit-identical either way.  The crops' bytes must not change between the two calls.
 *   - trexhip_load_weights, trexhip_set_identity_precision, a larger batch than the buffers hold, and trexhip_destroy drop the record; a second
 *     prepare call replaces it.
 *   - TREXHIP_OK without launching anything where the identify call's chain has no such part: another precision mode than TREXHIP_CNN_FP16X3,
 *     another size than 80 x 80 or another version than V118_3, a batch that takes another convolution chain (fewer than 3200 crops, 3 channels,
 *     unaligned crops), and a batch small enough for the captured-graph path (a captured chain is replayed whole).
 *   - With the stage timers on, the prepared launches are bracketed as TREXHIP_STAGE_PREPARE and are no longer inside the CONV2 / CONV3 brackets
 *     of the identify call that uses them.
 *   - Like an identify call it sizes the batch buffers for n: a prepare with a larger n than any call before reallocates them (and drops the
 *     captured chains that point into them).
 *   - The prepared kernels write the words the skip statistics read (trexhip_identify_skip_stats, _skipx_, _skip3_, _skip3x_, _fc1_ and
 *     _bgrow_stats): from the prepare call on these report the PREPARED batch, not the last identify call's.  Read a call's statistics
 *     before preparing the next one.
 * trexhip_identify_prepare_stats: records made by prepare calls on this context so far, and how many of them an identify call found and used
 * (a caller checks with it that its two calls do match: a mismatch costs the overlap in silence, never a bit).  Either pointer may be NULL.
 * (ABI 26) */
int trexhip_identify_prepare_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n);
int trexhip_identify_prepare_stats(trexhip_ctx* ctx, uint32_t* records, uint32_t* hits);
int trexhip_identify(trexhip_ctx* ctx, const uint8_t* crops, int32_t n, float* probs);
/* What the fp16 range guard of the LAST identify call on this context did (waits for the context's stream): *rerun_crops = crops
 * whose layer stack was re-run by the BF16X6 kernels (0 = none; the whole batch when the flag came from a kernel that does not
 * know the crop: *whole_batch = 1 -- also when other crops WERE named in the same batch).  Per crop since round 5: one out-of-range crop no
 * longer re-runs the batch.  Two documented exceptions to "a crop's probabilities do not depend on its batch": (1) the fused conv1 + conv2 kernels
 * attribute an out-of-range value to the crops that share its pass -- the crop itself and at most one neighbour in the batch --, and (2) more than
 * 1024 named crops re-run the whole batch; a crop that is re-run although it was in range gets the BF16X6 result, which differs from its FP16X3
 * result by about 2e-6 on the softmax (both inside the 1e-4 bar).  The answer refers to the last identify call even if
 * trexhip_set_identity_precision was called since; zeros before the first call and behind a call in another precision mode.  No reference
 * counterpart (the reference's torch network has no range limit); either pointer may be NULL. */
int trexhip_identify_guard_stats(trexhip_ctx* ctx, uint32_t* rerun_crops, uint32_t* whole_batch);
/* Identity crops are mostly background rows, and from 3200 one-channel 80 x 80 crops on (FP16X3) the fused conv1 + conv2 kernel computes only
 * the passes (3 pooled rows of conv2's output) whose band of crop rows holds a non-zero byte; the rows of the other passes are copied from the
 * image of an all-zero crop, made when the weights are loaded.  The crops' bytes decide, on the device, in every call; the results are the bits
 * of a run that computes every pass.  A network whose all-zero crop leaves the fp16 range computes every pass.  The environment variable
 * TREXHIP_CONV_GEOM (a test hook read when the context is created; every value gives identical results) switches this off with bit 27 (value
 * 134217728); its bits 0-11 select the fp32-activation chain, bit 28 keeps conv1 and conv2 apart, bit 29 forces this kernel at any batch size,
 * bit 30 the older fused kernel.
 * What the last such call did (waits for the context's stream): *passes of the batch, *listed of them computed, *bytes_filled of conv2's output
 * taken from that image instead of computed (copied for the dense conv3; read from the image in place by the listed conv3 below, which copies
 * nothing -- the count is the same either way); zeros before the first such call.  No reference counterpart; any pointer may be NULL.  (ABI 15) */
int trexhip_identify_skip_stats(trexhip_ctx* ctx, uint32_t* passes, uint32_t* listed, uint64_t* bytes_filled);

/* Where those passes are skipped, conv3 (k_conv5_wpair) computes only the row pairs -- two rows of its 20 x 20 map, pooled to one row of its
 * output -- that read a row of conv2's output with a blob in it, six listed pairs to a pass; the other row pairs are copied from the output of an
 * all-zero crop, made when the weights are loaded.  The crops' bytes decide, on the device, in every call, also whether the listed form pays at
 * all (a batch of noise lists every pair: the dense kernel runs then); the results are the bits of the dense kernel.  Bit 26 of TREXHIP_CONV_GEOM
 * (value 67108864) switches this off.  The listed form reads the background rows of conv2's output from the all-zero crop's image itself; bit 25
 * (value 33554432) has them copied into conv2's output first, as for the dense kernel.
 * What the last such call did (waits for the context's stream): *pairs of the batch (10 per crop), *listed of them to be computed, *passes the
 * listed form walked (0: the dense kernel ran), *bytes_filled of conv3's output copied instead; zeros before the first such call.  No reference
 * counterpart; any pointer may be NULL.  (ABI 16; since ABI 24 *passes counts by the row rule alone, six pairs to a pass, whatever windows the
 * call below gave its crops) */
int trexhip_identify_skip3_stats(trexhip_ctx* ctx, uint32_t* pairs, uint32_t* listed, uint32_t* passes, uint64_t* bytes_filled);

/* Where the listed form of conv3 reads the all-zero crop's image itself, a crop whose blob reaches at most 3 of the 5 column tiles of conv3's
 * map has its listed row pairs computed in windowed passes: ten row pairs of 3 tiles to a pass where a full-width pass holds six of 5; the 4
 * pooled columns of such a pair outside the window are copied from the all-zero crop's output.  The crops' bytes decide, on the device, in
 * every call (no crop has a window where the network's background leaves the fp16 range); the results are the bits of the dense kernel.  Bit 21
 * of TREXHIP_CONV_GEOM (value 2097152) switches this off: one list of full-width passes, as before.
 * What the last such call did (waits for the context's stream): *crops_windowed whose pairs went into windowed passes, *windowed_passes of them,
 * and the *full_passes of six pairs the other crops took; zeros where the dense kernel ran.  trexhip_identify_skip3_stats keeps counting by the
 * row rule alone: its *passes are the passes of six pairs that the listed pairs make, which is what ran before there were windows and under bit 21.
 * No reference counterpart; any pointer may be NULL.  (ABI 24; since ABI 27 *windowed_passes and *full_passes count passes of WHOLE pairs, ten and
 * six to a pass, whether the kernel walked those or the passes of the call below -- as *passes of trexhip_identify_skip3_stats does.  The choice
 * between the listed and the dense form is made on these counts.) */
int trexhip_identify_skip3x_stats(trexhip_ctx* ctx, uint32_t* crops_windowed, uint32_t* windowed_passes, uint32_t* full_passes);

/* A pass of the listed conv3 kernel has 64 tile slots, and whole pairs fill 60 of them (6 pairs of 10 tiles, 10 pairs of a window's 6).  Since
 * ABI 27 a listed pass, full-width or windowed, is up to 64 CONSECUTIVE tiles of its list's pair sequence instead: it may begin and end at any
 * even tile of a pair, and a pair cut between two passes is computed in part by each.  The results are the bits of the passes of whole pairs,
 * which bit 20 of TREXHIP_CONV_GEOM (value 1048576) brings back.
 * What the last such call did (waits for the context's stream): the *windowed_passes and *full_passes that the two listed instances walked --
 * under bit 20 the numbers of trexhip_identify_skip3x_stats --; zeros where the dense kernel ran.  No reference counterpart; either pointer may
 * be NULL.  (ABI 27) */
int trexhip_identify_skip3_ran(trexhip_ctx* ctx, uint32_t* windowed_passes, uint32_t* full_passes);

/* Above 3200 one-channel 80x80 crops in TREXHIP_CNN_FP16X3, where the skipping above is on, a crop whose blob fits 8 of the 10 column tiles of
 * conv2's output takes windowed passes of the fused conv1+conv2 kernel: 8 tiles of up to 4 output row pairs of that crop alone, the rest taken
 * from images of an all-zero crop made when the weights are loaded; the other crops (and every crop of a network whose background leaves the
 * fp16 range) take the full-width passes as before.  The crops' bytes decide, on the device, in every call; the results are the bits of the
 * full-width kernel.  Bit 23 of TREXHIP_CONV_GEOM (value 8388608) switches this off: no crop gets a window, the same preparation kernels
 * make the one list of full-width passes.
 * What the last such call did (waits for the context's stream): *crops_windowed that took windowed passes, *windowed_passes of them, and the
 * aligned *full_passes the other crops took; zeros where the windowed form did not run.  trexhip_identify_skip_stats keeps counting by the row
 * rule alone.  No reference counterpart; any pointer may be NULL.  (ABI 22) */
int trexhip_identify_skipx_stats(trexhip_ctx* ctx, uint32_t* crops_windowed, uint32_t* windowed_passes, uint32_t* full_passes);

/* A windowed pass reads 12 rows of conv1's pooled output (40 per crop); those with no non-zero crop row under them -- the rows above and below
 * the blob -- hold one constant per channel, the same in every crop.  The windowed kernel does not make them: it reads them from a row made
 * once, when the weights are loaded, and makes only the others.  The results are the bits of the kernel that makes every row.  Bit 22 of TREXHIP_CONV_GEOM
 * (value 4194304) switches this off.
 * What the last call with windowed passes did (waits for the context's stream): *rows_read = the rows of conv1's pooled output its windowed
 * passes read, the passes of a crop counted as one run, *rows_made of them made; both 0 where every row is made (bit 22, bit 23).  No
 * reference counterpart; either pointer may be NULL.  (ABI 23) */
int trexhip_identify_bgrow_stats(trexhip_ctx* ctx, uint32_t* rows_read, uint32_t* rows_made);

/* Where conv3 lists row pairs and the batch has more than 1024 crops, fc1 -- ten split-K planes, plane q = row pair q of every crop -- computes
 * only the (crop, plane) rows whose row pair is listed; the head takes every other plane from the fc1 planes of an all-zero crop, made when the
 * weights are loaded, and the unlisted row pairs of conv3's output are no longer copied (bytes_filled above still counts them).  The results are
 * the bits of the dense fc1.  Bit 24 of TREXHIP_CONV_GEOM (value 16777216) switches this off.
 * What the last identify call did (waits for the context's stream): *rows = crop-plane rows of the batch (10 per crop), *listed of them
 * computed; both 0 where the call's fc1 was not the listed form.  No reference counterpart; either pointer may be NULL.  (ABI 21) */
int trexhip_identify_fc1_stats(trexhip_ctx* ctx, uint32_t* rows, uint32_t* listed);

/* ---- multi-GPU hand-off --------------------------------------------------------------------
 * Fixed-size per-blob identity table of the last batch, written to caller-owned device memory
 * (e.g. a torch tensor that is then all-gathered over RCCL/xGMI to rank 0, whose sequential matcher
 * consumes it -- Tracker::predicted, tracking/Tracker.cpp:237-247).  Row = 8 x u32 header
 * {global frame index = frame_base + frame, pv::bid, n_pixels, x0|y0<<16, x1|y1<<16, centroid x (f32),
 * centroid y (f32), valid} followed by `classes` float probabilities.  Rows >= n_blobs are zeroed. */
int trexhip_export_id_table_device(trexhip_ctx* ctx, const float* d_probs, int32_t n_blobs, int32_t classes,
                                   uint32_t frame_base, void* d_table, int32_t max_rows);
/* the full record of one blob for the all-gather: row = 16 x u32 {the 8 header words above, central second moments per pixel
 * mu20, mu11, mu02 (f32), Midline::len / angle / offset.x / offset.y (f32) and the midline status (-1 when no posture is handed in)}
 * + `classes` probabilities + midline_resolution x {x, y, height} (f32) of the normalised midline (zero unless status 0).
 * d_midline / d_midline_info = outputs of trexhip_midline_device, or both NULL. */
int trexhip_export_id_table_ex_device(trexhip_ctx* ctx, const float* d_probs, int32_t n_blobs, int32_t classes, uint32_t frame_base,
                                      const float* d_midline, const trexhip_midline_info* d_midline_info, int32_t midline_resolution,
                                      void* d_table, int32_t max_rows);

/* The collective of the frame-sharded path, owned by the library: one process per GPU, frames dealt to ranks in blocks, and after
 * every block each rank's table goes to rank 0 (grouped ncclSend / ncclRecv over RCCL -- xGMI inside a node -- on the context's
 * stream, i.e. ordered behind trexhip_export_id_table*_device): a GATHER, because only rank 0's sequential matcher reads the tables.
 *   trexhip_comm_unique_id   rank 0: 128 bytes (ncclUniqueId) to hand to every rank by whatever side channel the host program has
 *   trexhip_comm_create      every rank, collectively (ncclCommInitRank on the context's device); world = 1 needs no id and no RCCL
 *   trexhip_comm_gather_device  `bytes` from every rank's d_send land at d_recv_rank0 + rank * bytes on rank 0 (world x bytes there;
 *                            ignored on the other ranks).  Enqueued on the context's stream; trexhip_synchronize waits for it.
 *   trexhip_comm_gather_device_on  the same on the stream of ANOTHER context of the same device: software-pipelined contexts (one per
 *                            batch in flight) share ONE communicator -- one ncclCommInitRank per process instead of one per context.
 *                            RCCL orders the operations of a communicator by their issue order, so every rank must issue its gathers in
 *                            the same sequence (one host thread driving the contexts in a fixed rotation does).
 * RCCL is loaded with dlopen on first use (an instance already in the process is shared). */
typedef struct trexhip_comm trexhip_comm;
int trexhip_comm_unique_id(void* id128);
int trexhip_comm_create(trexhip_ctx* ctx, const void* id128, int32_t rank, int32_t world, trexhip_comm** out);
void trexhip_comm_destroy(trexhip_comm* comm);
int trexhip_comm_rank(trexhip_comm* comm);
int trexhip_comm_world(trexhip_comm* comm);
int trexhip_comm_gather_device(trexhip_comm* comm, const void* d_send, size_t bytes, void* d_recv_rank0);
int trexhip_comm_gather_device_on(trexhip_comm* comm, trexhip_ctx* stream_ctx, const void* d_send, size_t bytes, void* d_recv_rank0);
/* collective health check: an all-reduce (sum) of 1 over the communicator -> the number of ranks that took part (= world when every
 * rank of the frame-sharded job is alive and on this communicator); synchronous, on the communicator's context's stream */
int trexhip_comm_count_ranks(trexhip_comm* comm, int32_t* ranks_seen);

/* live HIP-event timing of the dominant kernels on the ctx stream (bench.py roofline):
 * stage ids TREXHIP_STAGE_* ; returns accumulated milliseconds and launch count since reset */
enum { TREXHIP_STAGE_ROWS = 0, TREXHIP_STAGE_SEGMENT_ALL = 1, TREXHIP_STAGE_CONV2 = 2, TREXHIP_STAGE_CONV3 = 3,
       TREXHIP_STAGE_CNN_ALL = 4, TREXHIP_STAGE_CROPS = 5, TREXHIP_STAGE_POSTURE = 6,
       /* host-pointer entry points (trexhip_segment, trexhip_segment_color): per FRAME, always collected -- host milliseconds spent copying
        * pageable tiles into the pinned ring, and DMA milliseconds (HIP events on the copy stream).  The two legs overlap each other. */
       TREXHIP_STAGE_UPLOAD_COPY = 8, TREXHIP_STAGE_UPLOAD_DMA = 9,
       /* the launches of trexhip_identify_prepare_device (ABI 26); an unprepared identify call keeps them inside CONV2 / CONV3 */
       TREXHIP_STAGE_PREPARE = 10, TREXHIP_STAGE_COUNT = 11 };
int trexhip_profile_enable(trexhip_ctx* ctx, int32_t on);
int trexhip_profile_read(trexhip_ctx* ctx, int32_t stage, double* total_ms, int64_t* launches);
int trexhip_profile_reset(trexhip_ctx* ctx);

/* ------------------------------------------------------------------------------------------------
 * Training step of the identity network.
 * Replaces the body of the batch loop of train(), Application/src/tracker/python/visual_recognition_torch.py:1137-1158
 * (forward in training mode, nn.CrossEntropyLoss, backward, torch.optim.Adam(lr).step -- criterion / optimizer :1420-1421), for
 * V118_3 (visual_identification_network_torch.py:184-258) in fp32: the reference's arithmetic on every device but 'cuda', where it
 * additionally wraps the step in autocast + GradScaler (:1066-1072).  What stays on the host side of the boundary, as in the
 * reference: epochs, validation, ReduceLROnPlateau (-> set_lr) and early stopping (:1160-1283).  The data loader with its
 * augmentation (:158-188, :1325-1336) may stay there too (trexhip_train_step takes what it yields), or run on the device:
 * trexhip_augment_device below writes the batch trexhip_train_step_device takes, from crops that never left HBM.
 *   trexhip_trainer_create     weights = the blob of trexhip_load_weights (state_dict order, running statistics included); the
 *                              trainer keeps parameters, gradients and Adam moments in HBM.  Any individual_image_size that
 *                              trexhip_load_weights takes trains: 8 <= W, H <= 256, square or not (TREXHIP_E_UNSUPPORTED outside);
 *                              every call below follows the trainer's size (trexhip_trainer_image_size).  80 x 80 runs the tuned
 *                              kernels in the `precision` asked for; every other size runs a generic chain in exact fp32 (fp32 MFMA
 *                              for conv2 / conv3 in all three roles) at BOTH values of `precision` -- the fp16 two-piece split is an
 *                              80 x 80 matter.  Every reduction has a fixed order at every size: the same inputs give the same bits
 *   trexhip_train_step_device  d_inputs [n][H][W][channels] float32 in [0, 255] (NHWC, what TRexImageDataset yields), d_targets
 *                              [n] class indices.  d_keep_masks: null = the library draws the dropout masks (counter-based hash of
 *                              seed, step, index); else n*16 + n*64 + n*128 + n*100 bytes, 1 = keep: the masks of Dropout2d after
 *                              block 1, 2, 3 ([n][C]) and of the Dropout after fc1 ([n][100]) -- how the parity tests inject what
 *                              the reference drew.  loss / correct (host, optional): mean cross entropy and the number of samples
 *                              whose arg-max equals the target; passing either makes the call synchronise.  A target outside
 *                              0..classes-1 (train() asserts it, :1112) is flagged by the device: that call (if it synchronises)
 *                              and every later read / export return TREXHIP_E_INVALID.  The step is ordered on the context's
 *                              stream like every other call; inside, weight packing, mask drawing and the weight gradients run on a
 *                              second stream owned by the trainer and join the context's stream in front of the parameter update
 *   trexhip_trainer_export     the current weights as a blob for trexhip_load_weights (the reference hands its state_dict back)
 *   trexhip_trainer_read       one tensor in torch's layout; tensor = index in state_dict order (0 conv1.weight ... 23 fc2.bias,
 *                              running statistics included), kind 0 parameter, 1 gradient of the last step, 2 / 3 Adam moments
 * v100 and v110 (ABI 18).  A blob whose header names TREXHIP_NET_V100 or TREXHIP_NET_V110 (:328-382, :262-324) is parsed like
 * trexhip_load_weights parses it and gives a trainer of that version (trexhip_trainer_version): the same calls, the same resident path
 * (trexhip_augment_device, trexhip_train_predict_device, the validation and average calls).  Such a trainer runs one generic chain in exact
 * fp32 at every size, 80 x 80 included, at both values of `precision` (ChainTrainer, trex_amd/csrc/train_arch.hip), on the context's stream alone.  What differs:
 *   dropout rates              the architecture's: v100 0.25, 0.25, 0.25, 0.5; v110 0.25 four times.  trexhip_train_params.dropout is V118_3's
 *                              field; it is range-checked and otherwise not read
 *   d_keep_masks               n*16 + n*64 + n*100 + n*100 bytes: conv3 has 100 channels
 *   v110 and n = 1             a training step is TREXHIP_E_INVALID before any launch and leaves the trainer unchanged (the reference's
 *                              BatchNorm raises "Expected more than 1 value per channel when training"); eval and predict take n = 1
 *   trexhip_trainer_read       the version's own state_dict order and torch's shapes (trex_amd/weights.py shapes(arch=...)): v100 has 10 tensors,
 *                              v110 26 (bn4's running statistics included); conv3 and fc1 have 100 channels
 *   trexhip_trainer_export     header word 6 names the version; the blob loads with trexhip_load_weights
 * v119 and v200 are refused with TREXHIP_E_UNSUPPORTED and a text that names the version.
 * The category network (ABI 20).  A 'TRXC' blob -- the blob of trexhip_categorize_load_weights, parsed by the same parser, so refused with the
 * same codes and field names: 1..1024 categories, 1 or 3 channels, 8..256 each way -- gives a trainer of the category network
 * (trex_learn_category.py:18-44, PyTorchModel, in train mode; trexhip_trainer_version: TREXHIP_NET_CATEGORY).  A category network has no life
 * outside training: there are no pretrained weights, Categorize.perform_training (:276-340) trains it on the crops the user labelled.  The
 * step restates the loop body :314-332 on a non-CUDA device, in fp32; on 'cuda' the reference adds autocast and a GradScaler (:297, :318-331),
 * whose arithmetic is not restated.  The same calls, the same resident path; one generic chain in exact fp32 at every size and both values of
 * `precision` (the same ChainTrainer, trex_amd/csrc/train_arch.hip), on the context's stream alone, every reduction in a fixed order.  What differs:
 *   the network                x = byte / 127.5 - 1 (:289, a true fp32 division, then the subtraction), padded with zeros AFTER the normalisation;
 *                              three blocks of [conv 3x3 padding 1 -> BatchNorm2d (batch statistics over all n h w pixels, the odd last row and
 *                              column included) -> ReLU -> floor 2x2 max-pool -> element-wise Dropout(0.25)] with 16, 64, 100 channels (:22-36);
 *                              NCHW flatten; fc1 (100) -> ReLU -> Dropout(0.25) -> fc2 (categories) (:37-43); mean cross entropy; Adam with the
 *                              reference's defaults (:295: lr 1e-4 -- trexhip_train_params.lr -- and a batch of 32)
 *   inputs                     float32 [n][H][W][channels] in [0, 255] like every other trainer: the normalisation happens inside the first layer,
 *                              forward and in conv1's weight gradient.  trexhip_augment_device's plain path, trexhip_train_predict_device on uint8
 *                              crops and the validation calls work unchanged
 *   dropout                    0.25 four times; trexhip_train_params.dropout is range-checked and otherwise not read
 *   d_keep_masks               ELEMENT-wise ("Using Dropout instead of Dropout2d", :35): four planes back to back, 1 = keep, NHWC,
 *                              [n][h1][w1][16] [n][h2][w2][64] [n][h3][w3][100] [n][100] with (h_i, w_i) the pooled planes by successive floors
 *                              (h1 = H / 2, h2 = h1 / 2, h3 = h2 / 2); 4-byte aligned.  trexhip_trainer_keep_mask_bytes gives the size
 *   n = 1                      trains: block 3's convolution plane has at least 2 x 2 pixels at every legal size
 *   trexhip_trainer_read       the module's state_dict order and torch's shapes (trex_amd/weights.py category_shapes): 22 tensors, running
 *                              statistics included, without num_batches_tracked
 *   trexhip_trainer_export     a 'TRXC' blob that trexhip_categorize_load_weights takes; trexhip_load_weights keeps refusing it
 * What stays with the caller: the validation split, the "500 new samples" rule, the checkpoint file, classification_report.
 * ------------------------------------------------------------------------------------------------ */
#define TREXHIP_NET_CATEGORY 100      /* trexhip_trainer_version of a category trainer: not an identity network, outside the TREXHIP_NET_* of a blob's header */
typedef struct trexhip_trainer trexhip_trainer;
typedef struct {
    int32_t max_batch;          /* largest n of a step (VINetwork: 64..128, ml/VisualIdentification.cpp:112-118)               */
    float lr;                   /* learning_rate, 0.001 (visual_identification_network.py:151)                                */
    float beta1, beta2, eps;    /* torch.optim.Adam defaults 0.9, 0.999, 1e-8                                                */
    float bn_momentum;          /* nn.BatchNorm2d default 0.1                                                                */
    float dropout;              /* V118_3: 0.05 for all four dropout layers (visual_identification_network_torch.py:189-208).
                                   v100 / v110 use their architecture's rates and do not read it                              */
    int32_t precision;          /* (80 x 80; other sizes run exact fp32 at both values) arithmetic of the conv2 / conv3 forward, data-gradient and weight-gradient convolutions: 0 = fp16 two-piece split on the
                                   16-bit matrix cores (22-bit operands, fp32 accumulate, per-tensor power-of-two scales: the inference
                                   path's arithmetic), 1 = exact fp32 MFMA.  Everything else is fp32 either way                     */
    uint64_t seed;              /* of the library's own dropout masks                                                        */
} trexhip_train_params;
size_t trexhip_weight_blob_bytes(int32_t classes, int32_t channels);   /* of an 80 x 80 blob; a trainer exports as many bytes as the blob it was created from */
int trexhip_trainer_create(trexhip_ctx* ctx, const void* blob, size_t bytes, const trexhip_train_params* params, trexhip_trainer** out);
void trexhip_trainer_destroy(trexhip_trainer* trainer);
int trexhip_trainer_set_lr(trexhip_trainer* trainer, float lr);
int64_t trexhip_trainer_steps(trexhip_trainer* trainer);
/* the individual_image_size of the blob the trainer was created from: what every batch, crop and exported blob of this trainer has (ABI 14) */
int trexhip_trainer_image_size(trexhip_trainer* trainer, int32_t* width, int32_t* height);
/* the TREXHIP_NET_* of the blob the trainer was created from: V118_3, V100 or V110 (ABI 18); TREXHIP_NET_CATEGORY for a 'TRXC' blob (ABI 20) */
int trexhip_trainer_version(trexhip_trainer* trainer, int32_t* version);
/* bytes of the d_keep_masks of a step of n samples, for any trainer: V118_3 n * 308, v100 / v110 n * 280, the category network
 * n * (h1 w1 16 + h2 w2 64 + h3 w3 100 + 100).  The three layouts differ; callers need not restate them.  0 for a null trainer or n < 0 (ABI 20) */
size_t trexhip_trainer_keep_mask_bytes(trexhip_trainer* trainer, int32_t n);
int trexhip_train_step_device(trexhip_trainer* trainer, const float* d_inputs, const int32_t* d_targets, int32_t n, const uint8_t* d_keep_masks,
                              float* loss, int32_t* correct);
/* model.eval() forward + mean cross entropy + arg-max count of one validation batch (train(), :1171-1190: what ReduceLROnPlateau and the
 * early-stopping callback are fed); running statistics, nothing dropped; changes nothing in the trainer */
int trexhip_train_eval_device(trexhip_trainer* trainer, const float* d_inputs, const int32_t* d_targets, int32_t n, float* loss, int32_t* correct);
int trexhip_train_eval(trexhip_trainer* trainer, const float* inputs, const int32_t* targets, int32_t n, float* loss, int32_t* correct);
/* the same step from host memory (what the reference's DataLoader yields); targets are range-checked like train() does (:1112) */
int trexhip_train_step(trexhip_trainer* trainer, const float* inputs, const int32_t* targets, int32_t n, const uint8_t* keep_masks, float* loss,
                       int32_t* correct);
/* Softmax rows of any number of crops from the weights as they stand in the trainer: what ValidationCallback.plot_comparison_raw
 * (visual_recognition_torch.py:406-451) and estimate_uniqueness() -> Accumulation::calculate_uniqueness (ui/Accumulation.cpp:767-879) get from
 * predict_numpy at the end of every epoch, without exporting the weights to the inference context.  d_crops uint8 [n][H][W][channels] at the trainer's size
 * (what the crop calls and the resident pool hold), d_probs float32 [n][classes]: model.eval(), running statistics, nothing dropped, in the
 * trainer's `precision`.  Any n >= 1: the call walks the crops in chunks of at most max_batch through the trainer's own buffers (a row does
 * not depend on its chunk).  Ordered on the context's stream, NO host synchronisation; parameters, moments, running statistics and the step
 * counter stay as they are */
int trexhip_train_predict_device(trexhip_trainer* trainer, const uint8_t* d_crops, int32_t n, float* d_probs);
int trexhip_trainer_read(trexhip_trainer* trainer, int32_t tensor, int32_t kind, float* out, size_t count);
int trexhip_trainer_export(trexhip_trainer* trainer, void* blob, size_t capacity, size_t* bytes);

/* ------------------------------------------------------------------------------------------------
 * The training loader on the device.  Replaces TRexImageDataset.__getitem__ + DataLoader(num_workers=0)
 * (visual_recognition_torch.py:158-194, :1325-1337, :1391-1402): a resident pool of uint8 crops (what the crop calls write) and an
 * index list become the float32 [n][H][W][C] batch in [0, 255] that trexhip_train_step_device takes, augmented as the reference's
 * transform does it: torchvision RandomAffine(degrees=5, translate=(move_range, move_range)) -- nearest neighbour, fill 0, about the
 * image centre, angle clockwise -- then ColorJitter(brightness, contrast, saturation = 0.85..1.15, hue = +-0.05) on x = byte / 255
 * in a random order of its four operations, every operation ending in clamp(0, 1); output clamp(x, 0, 1) * 255 (:186).
 *   d_pool            [pool_size][H][W][C] uint8;  d_out [n][H][W][C] float32;  sample i of the batch = pool entry indices[i]
 *   indices           HOST array of n entries, NULL = 0 .. n-1; checked before anything is launched: an entry outside
 *                     0 .. pool_size-1 returns TREXHIP_E_INVALID and nothing runs
 *   ap                NULL = the validation loader (transform=None): d_out = float(pool byte) exactly, no draws
 *   d_draws           device, [n] trexhip_augment_draw.  draws_given != 0: sample i uses d_draws[i] (how the parity tests inject what the
 *                     reference drew, like d_keep_masks).  draws_given == 0: the kernel draws per sample from a counter-based hash of
 *                     (ap->seed, counter, i, field) -- angle ~ U(-degrees, degrees), tx = round_half_even(U(-translate_x W, translate_x W)),
 *                     ty likewise, the four factors uniform in their ranges, a uniformly random order (RandomAffine.get_params,
 *                     ColorJitter.get_params) -- and writes what it drew to d_draws when that is not NULL.  Hand a new `counter` per call.
 *   d_pool_targets / d_targets_out   optional, both or neither: d_targets_out[i] = d_pool_targets[indices[i]]
 * Sizes: 8 <= width, height <= 256, channels 1 or 3 (TREXHIP_E_UNSUPPORTED otherwise), n >= 1.  Saturation and hue are the identity for
 * one channel; the contrast mean is the mean of the image as it stands at that point (of its gray value for three channels).
 * One kernel launch on the context's stream, no synchronisation; a sample's output depends on nothing but its pool entry and its draw. */
typedef struct {
    float degrees;                       /* 5: angle ~ U(-degrees, degrees)                                  */
    float translate_x, translate_y;      /* move_range = min(0.05, 2 / min(W, H))   (:1301)                  */
    float brightness_lo, brightness_hi;  /* 0.85, 1.15                                                       */
    float contrast_lo, contrast_hi;      /* 0.85, 1.15                                                       */
    float saturation_lo, saturation_hi;  /* 0.85, 1.15                                                       */
    float hue_lo, hue_hi;                /* -0.05, 0.05                                                      */
    uint64_t seed;
} trexhip_augment_params;
typedef struct {                         /* one sample's draw, 32 bytes                                      */
    float angle; int32_t tx, ty;         /* degrees; whole pixels                                            */
    float brightness, contrast, saturation, hue;
    int32_t order;                       /* application order of 0 brightness, 1 contrast, 2 saturation, 3 hue: 2 bits each, first
                                            operation in the lowest bits (identity order = 0xE4)                */
} trexhip_augment_draw;
void trexhip_default_augment_params(trexhip_augment_params* p, int32_t width, int32_t height);
int trexhip_augment_device(trexhip_ctx* ctx, const trexhip_augment_params* ap, const uint8_t* d_pool, const int32_t* d_pool_targets,
                           int32_t pool_size, const int32_t* indices, int32_t n, int32_t width, int32_t height, int32_t channels,
                           trexhip_augment_draw* d_draws, int32_t draws_given, uint64_t counter, float* d_out, int32_t* d_targets_out);

/* ------------------------------------------------------------------------------------------------
 * Validation metrics of identity training on probabilities that are in HBM (trexhip_train_predict_device's rows, or
 * trexhip_identify_device's for the shipped network): the two reductions ValidationCallback.evaluate
 * (visual_recognition_torch.py:493-543) steers acceptance and early stopping by.  One launch plus a finalise; the call synchronises,
 * because it returns host values.
 *   confusion matrix   confusion[target][argmax] += 1 over all n rows (needs d_targets).  Its diagonal over its row sums is column 3 of
 *                      plot_comparison_raw (:449, (y.argmax(axis=1) == i).sum() / len(y)).  argmax is np.argmax: the first index of the
 *                      maximum, the first NaN if the row holds one -- also for a row that has no identity in the sense below (an all-zero
 *                      row counts in column 0, as plot_comparison_raw would count it)
 *   uniqueness         Accumulation::calculate_uniqueness (ui/Accumulation.cpp:767-879) over n_frames ranges of rows, line by line:
 *       identity of a row (:804-814): max_p = 0, ids ascending, take id iff p > max_p: the first index wins a tie; a row with no entry
 *           > 0 (all zero, all negative, NaN) has no identity and adds nothing to its frame
 *       per frame: unique_percent_raw = distinct / float(length) in float32, 0 for an empty range (:822-824, :840); accum_p = float32 sum
 *           over the frame's distinct identities of the largest max_p each got, summed in ASCENDING IDENTITY ORDER (the reference
 *           iterates a hash_map, :827: its order is unspecified; this one is fixed so that results repeat);
 *           unique_percent = float(logistic(accum_p / float(distinct)) * raw) when distinct > 0, logistic(x) = 1 / (1 + exp(-x * M_PI)) * NORMAL
 *           in double, NORMAL = 1 + expf(-float(M_PI)) (:834-849); the frame is good iff distinct == length, so an empty one is (:852-858)
 *       across frames, in frame order: the double sums of both per-frame values (:841, :850), and per identity the float32 sum of its
 *           largest max_p over the frames it appeared in, divided by their number, 0 if it never appeared (:830-831, :865-870)
 *   frame_ranges       HOST [n_frames][2] = {start, end} rows; may overlap and leave gaps.  Checked before anything is launched:
 *                      0 <= start <= end <= n, n_frames >= 1; 1 <= classes <= 1024; else TREXHIP_E_INVALID and nothing runs
 *   d_targets          device [n]; a target outside 0..classes-1 is flagged by the device: TREXHIP_E_INVALID, no output is written
 * Every output pointer is HOST memory and optional; without d_targets no confusion matrix is made, without frame_ranges no uniqueness.
 * Two calls on the same input give the same bytes: every floating-point sum has a fixed order, the confusion counts are integers. */
typedef struct {
    uint32_t good_frames, bad_frames;   /* Accumulation.cpp:852-858 */
    float    good_ratio;                /* float(good) / float(good + bad)          (:878, first element)  */
    float    mean_unique;               /* percentages / n_frames                    (:878, third element)  */
    float    mean_unique_raw;           /* rpercentages / n_frames                   (:875)                 */
} trexhip_uniqueness_result;
int trexhip_validation_metrics_device(trexhip_ctx* ctx, const float* d_probs, int32_t n, int32_t classes,
                                      const int32_t* d_targets,            /* [n] or NULL: no confusion matrix       */
                                      const int32_t* frame_ranges,         /* HOST [n_frames][2] = {start, end}, or NULL */
                                      int32_t n_frames,
                                      uint32_t* confusion,                 /* HOST [classes][classes], row = target, or NULL */
                                      trexhip_uniqueness_result* result,   /* HOST, or NULL                          */
                                      float* unique_percent,               /* HOST [n_frames] (:849), or NULL        */
                                      float* unique_percent_raw,           /* HOST [n_frames] (:840), or NULL        */
                                      float* uniqueness_per_class);        /* HOST [classes]  (:865-870), or NULL    */

/* ------------------------------------------------------------------------------------------------
 * Average probabilities per individual on rows that are in HBM: VINetwork::paverages (ml/VisualIdentification.h:145-180), which
 * Accumulation::check_additional_range (ui/Accumulation.cpp:455-641) asks for once per candidate range, and the arg-max scan it runs
 * over every averaged row (:526-541).  Only n_ids x classes floats leave the device instead of n x classes.
 *   sum        values[k][c] = float32 sum of d_probs[i][c] over the rows i with d_ids[i] == k in ASCENDING ROW ORDER -- the order of the
 *              reference's loop (std::transform(..., std::plus<>{}), :159-175) -- then ONE correctly rounded division by float(samples[k])
 *              (:177-178).  The chain of one (id, class) is never split or re-associated: the result equals the host loop bit for bit.
 *   samples    samples[k] = the number of rows of k as a float (`float samples; ++samples`, :171); n <= 2^24 keeps it exact
 *   arg-max    max_p = 0, take index i iff v > max_p (:533-536): the first index wins a tie, a NaN is never taken, a row with nothing
 *              above 0 gives max_index -1 and max_p 0.  Taken on the device: who wants only the decision copies 8 * n_ids bytes
 *   d_ids      device [n], dense keys 0..n_ids-1 (the position of the individual's id in the ordered std::map of the reference).  A key
 *              without rows gets samples 0, all-zero values (no division), max_index -1, max_p 0; the reference's map has no entry then.
 *              A key outside 0..n_ids-1 is flagged by the device: TREXHIP_E_INVALID, no output is written
 * Checked before anything is launched (TREXHIP_E_INVALID, nothing runs): 1 <= n <= 2^24, 1 <= classes <= 1024, 1 <= n_ids <= 65536,
 * d_probs and d_ids not NULL.  d_probs needs no alignment beyond a float's.  Every output pointer is HOST memory and optional.
 * Ordered on the context's stream; the call synchronises, because it returns host values, with one device-to-host copy.  No
 * floating-point atomics: two calls on the same input give the same bytes.  The rows of an id are found by one wave per (id, segment of
 * rows) reading the segment's ids: the work of that stage grows with n_ids x n -- it is made for ids that are individuals. */
int trexhip_class_averages_device(trexhip_ctx* ctx, const float* d_probs, int32_t n, int32_t classes,
                                  const int32_t* d_ids,                    /* device [n], dense keys 0..n_ids-1      */
                                  int32_t n_ids,
                                  float* samples,                          /* HOST [n_ids], or NULL                  */
                                  float* averages,                         /* HOST [n_ids][classes], or NULL         */
                                  int32_t* max_index,                      /* HOST [n_ids], or NULL                  */
                                  float* max_p);                           /* HOST [n_ids], or NULL                  */

/* ------------------------------------------------------------------------------------------------
 * Every individual's visual field on outlines that are in HBM: track::VisualField::calculate (tracking/VisualField.cpp:361-577) as
 * Individual::save_visual_field (tracking/Individual.cpp:2887-3010) and output_visual_fields ask for it, for a batch of frames and any
 * number of observers per frame in one call.  Per observer and eye a two-layer depth buffer of TREXHIP_VF_RESOLUTION bins over
 * +-RADIANS(130) around the eye's direction; every outline point of every individual of the frame, the observer itself included, enters
 * it as two lines.  Restated line by line:
 *   tesselate_outline (:339-359)      previous starts as the last outline point; an edge longer than max_distance gets the points
 *                                     previous + direction * i * max_distance for int i = 1; i < N - 1, N = L / max_distance + 0.5 in double
 *   the loop over the active individuals (:526-576)   an entry is used iff posture_row >= 0, its posture info has n_outline > 0 and its
 *                                     tail index is not -1 (:552); entries are applied in list order, the observer's own like any other;
 *                                     right_side = T + 1, left_side = n - T from the TARGET's tail index T and the tessellated length n,
 *                                     then the replacements of :435-436
 *   add_line (:427-496)               per tessellated point i two records, (previous, pt) then (ptp, pt), previous = points[n - 1] and
 *                                     ptp = points[(n - 2) % n] to begin with; hd = (1 - |i - T_obs| / ((i > T_obs ? left : right) + 1)) * 255
 *                                     with the OBSERVER's tail index (the lambda captured the outer midline, :460; the inner one of :531 only
 *                                     shadows it for the two sides), so hd may leave [0, 255]; per eye line = pt + (pos - eye.pos),
 *                                     atan2 of both ends, project_angles_1d (:74-94) as written; rp = pt0 + pos if the FIRST projected value
 *                                     (after the swap) is >= 0, else pt1 + pos; d = squared distance from rp to the eye
 *   plot_projected_line (:96-150)     the x0 / x1 replacements in the order of :102-103, start = uint(max(0, x0)), end = uint(min(512,
 *                                     ceil(x1))), bins i <= end && i < 512, the two-layer update with its id tests and the invalidation of
 *                                     layer 2 behind a self hit; fov = uchar(SQR(1 - min(1, max(0, d / max_d))) * 255); points as float(rp)
 * Per eye the records are applied in the order (entry, i, pair): layer 2 is not a function of a minimum, the order is the algorithm.
 * Every operation but the two atan2 gives the bits of tests/visual_field_ref.py and HipVisualField::cast_host; atan2 is the device
 * library's (the reference's is libm's; neither is correctly rounded), so a result can differ only where a projected value sits within
 * an ulp of an integer or of a field-of-view end.
 *   d_outline, d_posture_info   what trexhip_posture_device / trexhip_posture_auto_device wrote (row length max_points); the outline of
 *                               `virtual_frame` (:538-548): the look-back over max_back_view frames is the caller's, it names the row of
 *                               whichever frame's outline it found
 *   d_frame_entries             [n_frames + 1] ascending offsets into d_entries, [0] = 0, [n_frames] <= n_entries
 *   d_entries                   per frame the individuals in the order of Tracker::active_individuals(frame)
 *   d_observers                 one VisualField object each; eye positions and angles as VisualField::generate_eyes returns them
 * Outputs: device memory, [n_observers][2 eyes][TREXHIP_VF_LAYERS][TREXHIP_VF_RESOLUTION] each -- per eye the members _depth,
 * _visible_ids, _visible_points (float2), _fov, _visible_head_distance in the shape save_visual_field writes -- and d_status
 * [n_observers]; any of them may be NULL.  Initial values are eye::eye()'s (VisualField.h:37-43): depth FLT_MAX as a double, ids -1,
 * points 0, fov 0, head distance -1.
 *   d_status   0 ok;  1 the observer's own entry is not used (no outline, no tail index): nothing but the initial values is written;
 *              2 an entry of its frame needs more than max_tess_points tessellated points: every observer of that frame gets the initial
 *                values only -- the frame is flagged, nothing is half-done; the other frames of the call are complete
 * Refused with TREXHIP_E_INVALID: negative counts, max_tess_points < max_points or max_points < 1, offsets that do not ascend from 0 or
 * pass n_entries, an observer whose frame is outside 0..n_frames-1 or whose entry lies outside its frame's range (found by the device
 * before anything is written; for that the call synchronises once at its end).  Otherwise ordered on the context's stream; scratch for
 * the tessellated outlines (n_entries x max_tess_points x 16 bytes) is kept in the context and grown on demand.
 * Not in this call: generate_eyes (:203-337: commons' LineSegmentsIntersect, and its history smoothing is tracker state; it is a public
 * static of the reference, the caller hands over its result), visual_field_shapes (:498-522: commons' poly_convex_hull),
 * gui_pose_smoothing > 0 (:382-383), and the look-back named above.
 * UNPINNED (the arithmetic is the un-vendored commons'; each reading is stated here and in DESIGN.md):
 *   Vec2 arithmetic in tesselate_outline   direction = pt - previous, L = sqrtf(x * x + y * y), direction /= L and
 *                                          previous + (direction * float(i)) * float(max_distance) are float32 operations, each rounded
 *                                          on its own; L > max_distance and N are evaluated in double; each point is then widened
 *   atan2(Vec64)                           atan2(v.y, v.x)
 *   long_t                                 int32_t
 *   RADIANS(130)                           130 * (M_PI / 180) in double */
#define TREXHIP_VF_RESOLUTION 512   /* VisualField::field_resolution */
#define TREXHIP_VF_LAYERS     2     /* VisualField::layers */
#define TREXHIP_VF_CHUNK_RECORDS 512   /* records one workgroup computes per step (one per thread); an entry is walked in steps of this many */
#define TREXHIP_VF_LDS_RECORDS  1024   /* records that wait in LDS before the bins apply them */
typedef struct trexhip_vf_params {
    double  max_d;            /* SQR(average.cols) + SQR(average.rows); default: the context's width, height */
    double  max_distance;     /* tesselate_outline's default argument: 5 */
    int32_t max_points;       /* row length of d_outline (the posture call's max_points) */
    int32_t max_tess_points;  /* capacity per entry of the tessellated outline */
} trexhip_vf_params;
typedef struct trexhip_vf_entry {    /* one individual of one frame, in the order of Tracker::active_individuals(frame) */
    int32_t id;               /* Identity::ID() */
    int32_t posture_row;      /* row of d_outline / d_posture_info (the outline of `virtual_frame`); -1: no outline, skipped */
    float   pos_x, pos_y;     /* bounds().pos() of that blob */
    int32_t flags;            /* bit 0: the midline was turned round (_inverted_because_previous): use head_index as the tail */
    int32_t reserved;
} trexhip_vf_entry;
typedef struct trexhip_vf_observer { /* one VisualField object */
    int32_t frame, entry;     /* index into d_frame_entries; index of its own entry (absolute) */
    double  eye_x[2], eye_y[2], eye_angle[2];   /* eye::pos, eye::angle as generate_eyes returns them (angle already corrected to (-pi, pi]) */
} trexhip_vf_observer;
void trexhip_default_vf_params(trexhip_ctx* ctx, trexhip_vf_params* p);
int trexhip_visual_field_device(trexhip_ctx* ctx, const trexhip_vf_params* vp,
        const float* d_outline, const trexhip_posture_info* d_posture_info,
        const int32_t* d_frame_entries /* [n_frames + 1] prefix offsets */, int32_t n_frames,
        const trexhip_vf_entry* d_entries, int32_t n_entries,
        const trexhip_vf_observer* d_observers, int32_t n_observers,
        double* d_depth, int32_t* d_ids, float* d_points /* float2 */, uint8_t* d_fov, double* d_head_distance,
        int32_t* d_status /* [n_observers] */);

/* ------------------------------------------------------------------------------------------------
 * Categorisation (ABI 19): TRex's second network, and the reduction of its labels per tracklet, on crops that are in HBM.
 *
 * The network is trex_learn_category.py:18-44 (PyTorchModel) in eval mode: x = crop / 127.5 - 1 (:289, :435; a true fp32 division, then an fp32
 * subtraction), three times [conv 3x3 padding 1 -> BatchNorm2d -> ReLU -> floor 2x2 max-pool] with 16, 64 and 100 channels -- the zero padding is
 * applied to the NORMALISED image --, the NCHW flatten, fc1 (100) -> ReLU -> fc2 (categories); label = argmax(softmax(logits)) (:441), the first
 * maximum.  It takes the same individual_image_size crops as the identity network (CategorizeDatastore.cpp:1185-1245), uint8 NHWC [n][H][W][C].
 * A context holds it BESIDE the identity network: loading, reloading or calling either one leaves the other and its results untouched, and nothing
 * is allocated for it before trexhip_categorize_load_weights.  Sizes 8..256 each way (square or not), 1 or 3 channels, 1..1024 categories.
 * The chain is the generic one of the v100..v200 identity networks (first layer and fc1 exact fp32, conv2 / conv3 in the arithmetic mode of
 * trexhip_set_identity_precision with its range guard, crops walked in chunks; a crop's row does not depend on n or on where it stands); a
 * category call adds nothing to trexhip_identify_guard_stats or to the identity stages of the profile.
 *
 * trexhip_categorize_load_weights  replaces model.load_state_dict(npz['model_state']) (trex_learn_category.py:232-233).  The blob
 *     (trex_amd/weights.py pack_category_blob; tools/convert_category_weights.py makes it from a checkpoint): 8 x int32 header {magic 'TRXC', 1,
 *     categories, width, height, channels, 0, 0}, then the float32 tensors in state_dict order.  A blob with a bad size, magic, version or range is
 *     refused with the field named in trexhip_last_error(), and the loaded category network stays.  An identity blob ('TRXW') is refused here, and
 *     trexhip_load_weights refuses a category blob, by the magic.
 * trexhip_categorize_info          the loaded network's categories, channels and size; zeros without weights.  Any pointer may be NULL.
 * trexhip_categorize_blob_bytes    bytes of the blob for that network; 0 outside the ranges above.  No reference counterpart.
 * trexhip_categorize_device        replaces Categorize.predict (trex_learn_category.py:398-443) behind py::set_variable("images", ..) +
 *     py::run(module, "predict") + receive (ui/Categorize.cpp:730-761): d_labels[n] = the category of each crop; d_probs [n][categories] (the softmax
 *     rows) and d_logits [n][categories] are optional.  Ordered on the context's stream, does not synchronise.
 * trexhip_categorize               the same from host crops to host labels (includes the copies, synchronises).
 * n = 0 is a no-op that returns TREXHIP_OK; a call without category weights is TREXHIP_E_INVALID and says so. */
int trexhip_categorize_load_weights(trexhip_ctx* ctx, const void* blob, size_t bytes);
int trexhip_categorize_info(trexhip_ctx* ctx, int32_t* categories, int32_t* channels, int32_t* width, int32_t* height);
size_t trexhip_categorize_blob_bytes(int32_t categories, int32_t channels, int32_t width, int32_t height);
int trexhip_categorize_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n, int32_t* d_labels, float* d_probs /* or NULL */, float* d_logits /* or NULL */);
int trexhip_categorize(trexhip_ctx* ctx, const uint8_t* crops, int32_t n, int32_t* labels);
/* The labels of a tracklet's rows reduced to the tracklet's label: DataStore::label_averaged (CategorizeDatastore.cpp:513-594, the counting
 * :555-585) and the shares of a sample (CategorizeInterface.cpp:212-247), for every tracklet in one call.
 *   d_labels[n], d_tracklet[n]   a row's label and its tracklet, 0 <= tracklet < n_tracklets; rows of a tracklet may stand anywhere
 *   d_counts[T][categories]      uint32: rows of the tracklet with that label.  A negative label (none) is skipped; a label >= categories is
 *                                skipped and counted in *skipped (the reference warns and goes on)
 *   d_rows[T]                    uint32: every row handed in for the tracklet, skipped ones included
 *   d_label[T]                   the first maximum of the counts (std::max_element), -1 when that maximum is 0
 *   d_share[T][categories]       optional: counts / float(rows), one correctly rounded fp32 division; 0 for a tracklet without rows
 *   skipped                      HOST, optional: rows skipped for a label >= categories
 * Integer adds only: the result does not depend on the order of the rows or on the grid.  A tracklet id outside [0, n_tracklets) is
 * TREXHIP_E_INVALID and nothing is written: a checked pass runs first.  1 <= n_tracklets <= 2^24, 1 <= categories <= 1024; n = 0 returns
 * TREXHIP_OK and writes nothing but *skipped = 0.  Needs no category weights.  Ordered on the context's stream; the call synchronises. */
int trexhip_tracklet_labels_device(trexhip_ctx* ctx, const int32_t* d_labels, const int32_t* d_tracklet, int32_t n, int32_t n_tracklets, int32_t categories,
                                   uint32_t* d_counts, uint32_t* d_rows, int32_t* d_label, float* d_share /* or NULL */, uint32_t* skipped /* host, or NULL */);
/* Every tracklet's crops reduced to its median image: the last step of the output_tracklet_images export, hist_utils::init / addImage
 * (Application/src/tracker/ui/Export.cpp:78-154) driven by the loop over a tracklet's fixed-size images (Export.cpp:1287-1364), for every
 * tracklet in one call and on the crop pool the three crop calls write.
 *   d_crops [n][height][width][channels]   uint8.  1 channel is taken as it is, 3 channels (B, G, R) go through cv::COLOR_BGR2GRAY (:1320-1327):
 *                                (B*1868 + G*9617 + R*4899 + 8192) >> 14
 *   d_tracklet[n]                a row's tracklet, 0..n_tracklets-1, or -1 = the row belongs to none.  Rows may stand in any order and
 *                                tracklets may interleave
 *   d_median[T][height][width]   gray: per pixel the value addImage leaves after the tracklet's last image (:104-110) -- the smallest i whose
 *                                cumulative count exceeds rows / 2 = sorted[rows / 2], the upper median at an even count.  A tracklet without
 *                                rows gets the all-zero image init leaves (:145-153); one row gives that image (its gray) back
 *   d_rows[T]                    uint32: rows of each tracklet.  The reference stores a median only where this is > 1 (:1355): the caller's rule
 * Integer arithmetic only: two calls, or any permutation of the rows, give the same bytes.  A checked pass runs before any result is written:
 * an id outside [-1, n_tracklets) is TREXHIP_E_INVALID; a tracklet with more than 32767 rows is TREXHIP_E_UNSUPPORTED (the reference's bins
 * are `short`, :85-89; more is undefined there) and trexhip_last_error() names the tracklet and its count; nothing is written in either case.
 * 8 <= width, height <= 256 and channels 1 or 3, TREXHIP_E_UNSUPPORTED otherwise; 1 <= n_tracklets <= 2^24, 0 <= n <= 2^24.  n = 0 returns
 * TREXHIP_OK with d_rows and d_median zeroed.  d_crops and d_median need no alignment (dword loads and stores where both bases and the crop
 * size allow, bytes otherwise; same result).  Ordered on the context's stream; synchronises only to read the checked pass's flag. */
int trexhip_tracklet_medians_device(trexhip_ctx* ctx, const uint8_t* d_crops, int32_t n, int32_t width, int32_t height, int32_t channels,
                                    const int32_t* d_tracklet, int32_t n_tracklets, uint8_t* d_median, uint32_t* d_rows);

#ifdef __cplusplus
}
#endif
#endif
