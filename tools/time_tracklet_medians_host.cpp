// time_tracklet_medians_host.cpp -- the line-by-line host twin of the tracklet median (track::tracklet_images_host, trex_amd/host/HipTrackletImages.h:
// hist_utils::addImage of Export.cpp:91-116 per image) behind a C entry point, for tools/time_tracklet_medians.py.
// Pool rows [t * per_tracklet, (t + 1) * per_tracklet) are tracklet t of individual t; only the first `tracklets` of them are taken.
#include <chrono>
#include "../trex_amd/host/HipTrackletImages.h"

extern "C" double ttm_host_twin(const uint8_t* crops, int64_t n, int32_t width, int32_t height, int32_t channels, int32_t per_tracklet,
                                int32_t tracklets, uint8_t* medians /* [tracklets][height][width] */) {
    using Rows = track::TrackletRows<track::Idx_t, cmn::Range<cmn::Frame_t>>;
    std::vector<Rows> groups;
    for (int32_t t = 0; t < tracklets; ++t) {
        Rows r{track::Idx_t((uint32_t)t), cmn::Range<cmn::Frame_t>(cmn::Frame_t(0), cmn::Frame_t(per_tracklet - 1)), {}};
        for (int32_t i = 0; i < per_tracklet; ++i) r.rows.push_back(t * per_tracklet + i);
        groups.push_back(std::move(r));
    }
    const auto t0 = std::chrono::steady_clock::now();
    const auto out = track::tracklet_images_host(crops, (size_t)n, width, height, channels, groups);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (out.all_images.size() != (size_t)tracklets * width * height) return -1.0;
    std::memcpy(medians, out.all_images.data(), out.all_images.size());
    return seconds;
}
