// HipAccumulation.h -- the network-bound decision of Accumulation::check_additional_range (Application/src/tracker/ui/Accumulation.cpp:455-641)
// on libtrexhip, in two parts:
//   paverages_device(net, ids, images) -> std::map<Idx, HipVINetwork::Average>
//       VINetwork::paverages (ml/VisualIdentification.h:145-180, called at :510) with the rows reduced where they are, in HBM -- one
//       trexhip_identify_device and one trexhip_class_averages_device, then one copy of n_ids x classes floats -- instead of
//       probabilities(images) and the loop over n x classes floats on the host.  Equals HipVINetwork::paverages on the same input bit for bit.
//   decide_additional_range(averages, track_max_individuals, accumulation_tracklet_add_factor) -> RangeDecision
//       :520-640 line by line: the per-id arg-max, min_prob, the set of predicted ids, the "only one missing id" guess and the three
//       outcomes.  Pure host code; the two TRex globals are arguments.  Logging, end_a_step and the data generation in front of it
//       (:459-500: tracker state) stay with the caller.
#pragma once
#ifdef TREXHIP_WITH_TREX
#include <commons.pc.h>
#include <misc/Image.h>
#include <core/idx_t.h>
#else
#include "trex_types.h"
#endif
#include <algorithm>
#include <limits>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/trexhip.h"
#include "HipVINetwork.h"

namespace track {

template <typename Idx, typename ImagePtr>
inline std::map<Idx, HipVINetwork::Average> paverages_device(HipVINetwork& net, const std::vector<Idx>& ids, const std::vector<ImagePtr>& images) {
    auto check = [](int rc) { if (rc != 0) throw std::runtime_error(std::string("libtrexhip: ") + trexhip_last_error()); };
    if (!net.weights_loaded()) throw std::runtime_error("Network is not set.");
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
    const size_t rows = std::min(ids.size(), images.size());                  // the loop of :159 walks ids over the rows that exist
    if (rows == 0) return {};
    // the distinct ids in std::map order -> dense keys 0..n_ids-1: key k is the k-th entry of the reference's `averages`
    std::map<Idx, int32_t> key_of;
    for (size_t i = 0; i < rows; ++i) key_of.emplace(ids[i], 0);
    int32_t n_ids = 0;
    for (auto& kv : key_of) kv.second = n_ids++;
    std::vector<int32_t> keys(rows);
    for (size_t i = 0; i < rows; ++i) keys[i] = key_of.at(ids[i]);
    const int32_t n = (int32_t)images.size();
    void *d_crops = nullptr, *d_probs = nullptr, *d_keys = nullptr;
    struct Free { trexhip_ctx* c; void*& p; ~Free() { trexhip_device_free(c, p); } } f1{ctx, d_crops}, f2{ctx, d_probs}, f3{ctx, d_keys};
    check(trexhip_device_alloc(ctx, crops.size(), &d_crops));
    check(trexhip_device_alloc(ctx, (size_t)n * C * sizeof(float), &d_probs));
    check(trexhip_device_alloc(ctx, rows * sizeof(int32_t), &d_keys));
    check(trexhip_copy_to_device(ctx, d_crops, crops.data(), crops.size()));
    check(trexhip_copy_to_device(ctx, d_keys, keys.data(), rows * sizeof(int32_t)));
    check(trexhip_identify_device(ctx, static_cast<const uint8_t*>(d_crops), n, static_cast<float*>(d_probs), nullptr));
    std::vector<float> samples((size_t)n_ids), values((size_t)n_ids * C);
    check(trexhip_class_averages_device(ctx, static_cast<const float*>(d_probs), (int32_t)rows, C, static_cast<const int32_t*>(d_keys), n_ids, samples.data(),
                                        values.data(), nullptr, nullptr));
    std::map<Idx, HipVINetwork::Average> averages;
    for (const auto& kv : key_of) {
        const size_t k = (size_t)kv.second;
        if (samples[k] <= 0) continue;                                        // an id without rows has no entry in the reference's map
        HipVINetwork::Average& av = averages[kv.first];
        av.samples = samples[k];
        av.values.assign(values.begin() + k * C, values.begin() + (k + 1) * C);
    }
    return averages;
}

enum class RangeStatus { Acceptable, NoUniqueIDs, ProbabilityTooLow };

template <typename Idx>
struct RangeDecision {
    RangeStatus status = RangeStatus::NoUniqueIDs;
    std::map<Idx, Idx> max_indexes;          // my id -> predicted id, after the guess; what check_additional_range returns when the range is acceptable
    float min_prob = std::numeric_limits<float>::infinity();
};

// Idx has the surface of track::Idx_t (core/idx_t.h): Idx() is invalid, Idx(uint32_t), valid(), <, ==, !=, +
template <typename Idx>
inline RangeDecision<Idx> decide_additional_range(const std::map<Idx, HipVINetwork::Average>& averages, uint32_t track_max_individuals,
                                                  float accumulation_tracklet_add_factor) {
    const cmn::Float2_t pure_chance = cmn::Float2_t(1) / cmn::Float2_t(track_max_individuals);                 // :456
    const auto bar = pure_chance * cmn::Float2_t(accumulation_tracklet_add_factor);
    RangeDecision<Idx> out;
    std::map<Idx, Idx>& max_indexes = out.max_indexes;
    std::map<Idx, float> max_probs;
    for (const auto& [id, av] : averages) {                                                                    // :520-546
        int64_t max_index = -1;
        float max_p = 0;
        for (uint32_t i = 0; i < av.values.size(); ++i) {
            const auto v = av.values[i];
            if (v > max_p) { max_index = i; max_p = v; }
        }
        max_indexes[id] = max_index >= 0 ? Idx((uint32_t)max_index) : Idx();
        max_probs[id] = max_p;
    }
    std::set<Idx> unique_ids;                                                                                  // :550-557
    float& min_prob = out.min_prob;
    for (const auto& [my_id, p] : max_probs) min_prob = std::min(min_prob, p);
    for (const auto& [my_id, pred_id] : max_indexes)
        if (pred_id.valid()) unique_ids.insert(pred_id);

    if (unique_ids.size() + 1 == track_max_individuals && min_prob > bar) {                                    // :559-614
        // searching for consecutive numbers, finding the gap
        Idx missing_predicted_id(0);
        for (auto id : unique_ids) {
            if (id != missing_predicted_id) break;
            missing_predicted_id = missing_predicted_id + Idx(1);
        }
        // find out which one is the duplicate (this only works if we have one of course)
        Idx duplicate0, duplicate1;
        std::map<Idx, Idx> assign;
        for (const auto& [my_id, pred_id] : max_indexes) {
            if (!pred_id.valid()) continue;
            if (assign.count(pred_id)) {
                duplicate0 = my_id;
                duplicate1 = assign.at(pred_id);
                break;
            }
            assign[pred_id] = my_id;
        }
        if (duplicate0.valid() && duplicate1.valid()) {                                                        // else: only a warning (:597-598)
            if (max_probs.at(duplicate0) > max_probs.at(duplicate1)) max_indexes[duplicate1] = missing_predicted_id;
            else max_indexes[duplicate0] = missing_predicted_id;
            unique_ids.insert(missing_predicted_id);
        }
    }

    if (unique_ids.size() == track_max_individuals && min_prob > bar) out.status = RangeStatus::Acceptable;    // :616-619
    else if (unique_ids.size() != track_max_individuals) out.status = RangeStatus::NoUniqueIDs;               // :621-625
    else out.status = RangeStatus::ProbabilityTooLow;                                                          // :627-632: min_prob <= bar
    return out;
}

}  // namespace track
