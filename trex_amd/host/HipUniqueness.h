// HipUniqueness.h -- Accumulation::calculate_uniqueness (Application/src/tracker/ui/Accumulation.cpp:767-879) on libtrexhip:
// the images are predicted by the network of a HipVINetwork and the rows are reduced where they are, in HBM -- one
// trexhip_identify_device and one trexhip_validation_metrics_device, then one copy of the results -- instead of
// _network->probabilities(images) and the loop over predictions on the host.
//   calculate_uniqueness(net, images, map_indexes)
//       -> { float(good_frames) / float(good_frames + bad_frames), unique_percent per frame, percentages / n_frames }   (:878)
//   the signature and return meaning of the reference's (its leading bool and its lock guard have nothing to steer here; the per-frame
//   map is a std::map, ordered like map_indexes).  What the reference stores in _current_accumulation->_uniqueness_per_class
//   (:861-871) comes back through the optional last argument.
// One difference, documented in include/trexhip.h: accum_p is summed in ascending identity order (the reference iterates a hash_map).
#pragma once
#ifdef TREXHIP_WITH_TREX
#include <commons.pc.h>
#include <misc/Image.h>
#include <misc/frame_t.h>
#include <misc/ranges.h>
#else
#include "trex_types.h"
#endif
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>
#include "../../include/trexhip.h"
#include "HipVINetwork.h"

namespace track {

template <typename ImagePtr>
inline std::tuple<float, std::map<cmn::Frame_t, float>, float> calculate_uniqueness(HipVINetwork& net, const std::vector<ImagePtr>& images,
                                                                                   const std::map<cmn::Frame_t, cmn::Range<size_t>>& map_indexes,
                                                                                   std::vector<float>* uniqueness_per_class = nullptr) {
    auto check = [](int rc) { if (rc != 0) throw std::runtime_error(std::string("libtrexhip: ") + trexhip_last_error()); };
    if (!net.weights_loaded()) throw std::runtime_error("Network is not set.");                      // :773-774
    trexhip_ctx* ctx = net.context();
    const int C = net.num_classes();
    int32_t W = 0, H = 0;
    check(trexhip_network_image_size(ctx, &W, &H));
    const size_t per = (size_t)W * H * (size_t)trexhip_network_channels(ctx);
    std::vector<uint8_t> crops;
    crops.reserve(images.size() * per);
    for (const auto& im : images) {
        if (!im || im->size() != per || (int32_t)im->rows != H || (int32_t)im->cols != W) throw std::runtime_error("Invalid image (expected individual_image_size and the network's channels)");
        crops.insert(crops.end(), im->data(), im->data() + per);
    }
    std::vector<int32_t> ranges;
    ranges.reserve(map_indexes.size() * 2);
    for (const auto& kv : map_indexes) { ranges.push_back((int32_t)kv.second.start); ranges.push_back((int32_t)kv.second.end); }
    if (map_indexes.empty()) return {std::numeric_limits<float>::quiet_NaN(), {}, std::numeric_limits<float>::quiet_NaN()};                                     // 0 / 0 in the reference too
    const int32_t n = (int32_t)images.size();
    void *d_crops = nullptr, *d_probs = nullptr;
    struct Free { trexhip_ctx* c; void*& p; ~Free() { trexhip_device_free(c, p); } } f1{ctx, d_crops}, f2{ctx, d_probs};
    if (n > 0) {
        check(trexhip_device_alloc(ctx, crops.size(), &d_crops));
        check(trexhip_device_alloc(ctx, (size_t)n * C * sizeof(float), &d_probs));
        check(trexhip_copy_to_device(ctx, d_crops, crops.data(), crops.size()));
        check(trexhip_identify_device(ctx, static_cast<const uint8_t*>(d_crops), n, static_cast<float*>(d_probs), nullptr));
    }
    trexhip_uniqueness_result r{};
    std::vector<float> unique_percent(map_indexes.size());
    if (uniqueness_per_class) uniqueness_per_class->assign((size_t)C, 0.f);
    check(trexhip_validation_metrics_device(ctx, static_cast<const float*>(d_probs), n, C, nullptr, ranges.data(), (int32_t)map_indexes.size(), nullptr, &r,
                                            unique_percent.data(), nullptr, uniqueness_per_class ? uniqueness_per_class->data() : nullptr));
    std::map<cmn::Frame_t, float> per_frame;
    size_t k = 0;
    for (const auto& kv : map_indexes) per_frame[kv.first] = unique_percent[k++];
    return {r.good_ratio, per_frame, r.mean_unique};
}

}  // namespace track
