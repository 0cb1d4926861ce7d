// The host route of tools/time_prefilter.py, as a caller had to write it before trexhip_prefilter_device: re-threshold on the device, fetch
// the second table set, decide every blob on one host thread (track::HipPrefilter::host_policy), upload presumed_nr for the split search.
// Built by the tool into a small shared library next to libtrexhip and called through ctypes on the tool's own context.
#include <cstdint>
#include <vector>
#include "../trex_amd/host/HipPrefilter.h"

static trexhip_batch_result g_det;

extern "C" {

// the detect tables of the batch, fetched once: both routes start behind trexhip_fetch
int tp_prepare(trexhip_ctx* ctx) { return trexhip_fetch(ctx, &g_det); }

// counts [n_frames][3] = committed, big, filtered out; d_presumed: device [total detect blobs]
int tp_host_route(trexhip_ctx* ctx, int32_t track_threshold, int32_t method, int32_t track_threshold_2, float ratio_lo, float ratio_hi,
                  const double* ranges, int32_t n_ranges, const uint8_t* bg, int32_t width, double cm_per_pixel, int32_t* d_presumed,
                  int32_t* counts) {
    track::HipPrefilter::Settings st;
    st.track_threshold = track_threshold; st.method = method; st.track_threshold_2 = track_threshold_2;
    st.threshold_ratio_range = cmn::Range<float>(ratio_lo, ratio_hi);
    for (int32_t i = 0; i < n_ranges; ++i) st.track_size_filter.emplace_back(ranges[2 * i], ranges[2 * i + 1]);
    int rc = trexhip_rethreshold_device(ctx, track_threshold, method, ranges, n_ranges);
    if (rc) return rc;
    trexhip_batch_result sub;
    rc = trexhip_fetch_rethreshold(ctx, &sub);
    if (rc) return rc;
    const auto r = track::HipPrefilter::host_policy(st, g_det, sub, bg, (size_t)width, cm_per_pixel);
    for (size_t f = 0; f < r.frames.size(); ++f) {
        counts[3 * f] = (int32_t)r.frames[f].filtered.size(); counts[3 * f + 1] = (int32_t)r.frames[f].big.size();
        counts[3 * f + 2] = (int32_t)r.frames[f].filtered_out.size();
    }
    return r.presumed_nr.empty() ? 0 : trexhip_copy_to_device(ctx, d_presumed, r.presumed_nr.data(), r.presumed_nr.size() * sizeof(int32_t));
}

}
