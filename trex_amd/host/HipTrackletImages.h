// HipTrackletImages.h -- the median image per tracklet of the output_tracklet_images export (Application/src/tracker/ui/Export.cpp:1287-1364,
// fixed-size images: can_we_expect_fix_dimensions) on libtrexhip, and its host twin:
//   tracklet_images_device(ctx, d_crops, n, width, height, channels, tracklets) -> TrackletImages{all_images, all_ranges}
//       the crops stay where the crop calls wrote them, in HBM: one trexhip_tracklet_medians_device, then one copy of tracklets x H x W bytes,
//       instead of every crop over PCIe and hist_utils::addImage per image.  Equals tracklet_images_host on the same input byte for byte.
//   tracklet_images_host(crops, n, width, height, channels, tracklets) -> TrackletImages
//       the reference's loop on host crops: hist_utils::init / addImage (Export.cpp:78-154) line for line, `short` bins included, for the
//       tests and for callers without a device
// Both take the caller's grouping -- one entry per (individual id, range) with the pool rows of its images -- and give back what the loop
// appends to all_images and all_ranges (the `meta` array: id, range.start, range.end), in the order of the reference's
// std::map<Idx_t, std::map<Range<Frame_t>, ...>> queues (:917): by id, then by range; only tracklets with more than one image (:1355).
// Which frames of a tracklet are sampled (tracklet_max_images, :496-513) stays with the caller, as do the single-image arrays and the .npz
// files.  A tracklet of more than 32767 images is refused: the reference's bins are `short` (:85-89).
#pragma once
#ifdef TREXHIP_WITH_TREX
#include <commons.pc.h>
#include <misc/ranges.h>
#include <core/idx_t.h>
#else
#include "trex_types.h"
#endif
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>
#include "../../include/trexhip.h"

namespace track {

// one tracklet of one individual: queues[id][range] (:1024); rows = the places of its images in the crop pool
template <typename Idx, typename RangeT>
struct TrackletRows {
    Idx id;
    RangeT range;
    std::vector<int32_t> rows;
};

struct TrackletImages {
    std::vector<uint8_t> all_images;     // [kept][height][width] gray medians (:1358)
    std::vector<int32_t> all_ranges;     // [kept][3]: id, range.start, range.end (:1359-1361; long_t)
};

namespace hist_utils {
// Export.cpp:78-154 without OpenCV: Mat1b is rows x cols bytes
struct Mat1b {
    int rows = 0, cols = 0;
    std::vector<uint8_t> bytes;
    Mat1b() = default;
    Mat1b(int r, int c, uint8_t v) : rows(r), cols(c), bytes((size_t)r * c, v) {}
    uint8_t& operator()(int r, int c) { return bytes[(size_t)r * cols + c]; }
};

struct Hist {
    std::vector<short> h;
    int count;
    Hist() : h(256, 0), count(0) {}
};

inline void addImage(Mat1b& img, std::vector<std::vector<Hist>>& M, Mat1b& med) {
    if (img.rows != med.rows || img.cols != med.cols) throw std::invalid_argument("addImage: image and median differ in size");
    for (unsigned r = 0; r < (unsigned)img.rows; ++r) {
        for (unsigned c = 0; c < (unsigned)img.cols; ++c) {
            // Add pixel to histogram
            Hist& hist = M[r][c];
            ++hist.h[img((int)r, (int)c)];
            ++hist.count;

            // Compute median
            unsigned i;
            int n = hist.count / 2;
            for (i = 0; i < 256 && ((n -= hist.h[i]) >= 0); ++i);

            // 'i' is the median value
            med((int)r, (int)c) = (uint8_t)i;
        }
    }
}

inline void init(std::vector<std::vector<Hist>>& M, Mat1b& med, int rows, int cols) {
    med = Mat1b(rows, cols, (uint8_t)0);
    M.clear();
    M.resize((unsigned)rows);
    for (unsigned i = 0; i < (unsigned)rows; ++i) M[i].resize((unsigned)cols);
}
}  // namespace hist_utils

namespace tracklet_images_detail {
using Key = std::tuple<uint32_t, int32_t, int32_t>;   // id, range.start, range.end: the order of the two nested maps

// the caller's grouping in the reference's order; an entry given twice is one tracklet, as queues[id][range] is one queue
template <typename Idx, typename RangeT>
inline std::map<Key, std::vector<int32_t>> ordered(const std::vector<TrackletRows<Idx, RangeT>>& tracklets, size_t n) {
    std::map<Key, std::vector<int32_t>> out;
    std::vector<char> listed(n, 0);
    for (const auto& t : tracklets) {
        auto& rows = out[Key{(uint32_t)t.id.get(), (int32_t)t.range.start.get(), (int32_t)t.range.end.get()}];
        for (int32_t r : t.rows) {
            if (r < 0 || (size_t)r >= n) throw std::invalid_argument("tracklet row " + std::to_string(r) + " is outside the crop pool");
            if (listed[(size_t)r]) throw std::invalid_argument("crop pool row " + std::to_string(r) + " is listed twice");   // an image sits in one queue
            listed[(size_t)r] = 1;
            rows.push_back(r);
        }
    }
    return out;
}

inline void check_size(int32_t width, int32_t height, int32_t channels) {
    if (width < 8 || width > 256 || height < 8 || height > 256) throw std::invalid_argument("individual_image_size must be 8..256 each way");
    if (channels != 1 && channels != 3) throw std::invalid_argument("Invalid number of channels: " + std::to_string(channels));   // :1328
}
}  // namespace tracklet_images_detail

template <typename Idx, typename RangeT>
inline TrackletImages tracklet_images_host(const uint8_t* crops, size_t n, int32_t width, int32_t height, int32_t channels,
                                           const std::vector<TrackletRows<Idx, RangeT>>& tracklets) {
    tracklet_images_detail::check_size(width, height, channels);
    const size_t px = (size_t)width * height, per = px * channels;
    TrackletImages out;
    std::vector<std::vector<hist_utils::Hist>> M;   // histograms
    hist_utils::Mat1b med;                          // median image
    for (const auto& [key, rows] : tracklet_images_detail::ordered(tracklets, n)) {
        if (rows.size() > 32767) throw std::invalid_argument("a tracklet of " + std::to_string(rows.size()) + " images overflows the short bins");
        size_t image_count = 0;
        hist_utils::init(M, med, height, width);
        for (int32_t r : rows) {
            const uint8_t* image = crops + (size_t)r * per;
            hist_utils::Mat1b tmp(height, width, 0);
            if (channels == 1) std::memcpy(tmp.bytes.data(), image, px);
            else                                                        // cv::cvtColor(mat, tmp, cv::COLOR_BGR2GRAY) (:1326), 8-bit fixed point
                for (size_t i = 0; i < px; ++i)
                    tmp.bytes[i] = (uint8_t)((image[3 * i] * 1868u + image[3 * i + 1] * 9617u + image[3 * i + 2] * 4899u + 8192u) >> 14);
            hist_utils::addImage(tmp, M, med);
            ++image_count;
        }
        if (image_count > 1) {                                          // :1355
            out.all_images.insert(out.all_images.end(), med.bytes.begin(), med.bytes.end());
            out.all_ranges.push_back((int32_t)std::get<0>(key));
            out.all_ranges.push_back(std::get<1>(key));
            out.all_ranges.push_back(std::get<2>(key));
        }
    }
    return out;
}

// d_crops: device, uint8 [n][height][width][channels] (what trexhip_crops_device and its siblings wrote)
template <typename Idx, typename RangeT>
inline TrackletImages tracklet_images_device(trexhip_ctx* ctx, const void* d_crops, size_t n, int32_t width, int32_t height, int32_t channels,
                                             const std::vector<TrackletRows<Idx, RangeT>>& tracklets) {
    auto check = [](int rc) { if (rc != 0) throw std::runtime_error(std::string("libtrexhip: ") + trexhip_last_error()); };
    tracklet_images_detail::check_size(width, height, channels);
    const auto order = tracklet_images_detail::ordered(tracklets, n);
    TrackletImages out;
    if (order.empty()) return out;
    std::vector<int32_t> tracklet_of(n, -1);                            // a pool row outside every tracklet takes no part
    int32_t T = 0;
    for (const auto& [key, rows] : order) {
        for (int32_t r : rows) tracklet_of[(size_t)r] = T;
        ++T;
    }
    const size_t px = (size_t)width * height;
    void *d_tracklet = nullptr, *d_median = nullptr, *d_rows = nullptr;
    struct Free { trexhip_ctx* c; void*& p; ~Free() { trexhip_device_free(c, p); } } f1{ctx, d_tracklet}, f2{ctx, d_median}, f3{ctx, d_rows};
    check(trexhip_device_alloc(ctx, (n ? n : 1) * sizeof(int32_t), &d_tracklet));
    check(trexhip_device_alloc(ctx, (size_t)T * px, &d_median));
    check(trexhip_device_alloc(ctx, (size_t)T * sizeof(uint32_t), &d_rows));
    if (n) check(trexhip_copy_to_device(ctx, d_tracklet, tracklet_of.data(), n * sizeof(int32_t)));
    check(trexhip_tracklet_medians_device(ctx, static_cast<const uint8_t*>(d_crops), (int32_t)n, width, height, channels,
                                          static_cast<const int32_t*>(d_tracklet), T, static_cast<uint8_t*>(d_median), static_cast<uint32_t*>(d_rows)));
    std::vector<uint8_t> medians((size_t)T * px);
    std::vector<uint32_t> counts((size_t)T);
    check(trexhip_copy_to_host(ctx, medians.data(), d_median, medians.size()));
    check(trexhip_copy_to_host(ctx, counts.data(), d_rows, counts.size() * sizeof(uint32_t)));
    size_t t = 0;
    for (const auto& [key, rows] : order) {
        if (counts[t] != rows.size()) throw std::runtime_error("trexhip_tracklet_medians_device counted other rows than were listed");
        if (counts[t] > 1) {                                            // :1355
            out.all_images.insert(out.all_images.end(), medians.begin() + t * px, medians.begin() + (t + 1) * px);
            out.all_ranges.push_back((int32_t)std::get<0>(key));
            out.all_ranges.push_back(std::get<1>(key));
            out.all_ranges.push_back(std::get<2>(key));
        }
        ++t;
    }
    return out;
}

}  // namespace track
