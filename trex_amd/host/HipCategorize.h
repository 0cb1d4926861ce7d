// HipCategorize.h -- TRex's categorisation on libtrexhip, in the manner of HipAccumulation.h:
//   HipCategorize(ctx)                the category network lives in a context BESIDE the identity network: hand in HipVINetwork::context() (or any
//                                     trexhip_ctx) and both networks share one device context
//   load_weights(blob, bytes)         Categorize.load (trex_learn_category.py:195-233) from a blob of tools/convert_category_weights.py
//   predict(images) -> vector<float>  what `receive` gets at ui/Categorize.cpp:730-761 behind py::set_variable("images", ..) + py::run(module,
//                                     "predict"): one label per image, as a float (the reference receives std::vector<float>)
//   label_averaged(labels, tracklet, n_tracklets) -> Votes
//                                     DataStore::label_averaged (CategorizeDatastore.cpp:555-585) and a sample's shares (CategorizeInterface.cpp:
//                                     212-247) for every tracklet at once, reduced on the device (trexhip_tracklet_labels_device)
//   label_averaged_host(...)          its host twin, line by line; equal byte for byte (tests/cpp/test_categorize.cpp)
//   sample_rows(size, first_frame, sample_rate, min_samples)
//                                     which rows of a tracklet are predicted at all (DataStore::temporary, CategorizeDatastore.cpp:1103-1152).
//                                     Pure host code.
//   HipCategorize::Trainer(ctx, blob, bytes, max_batch, lr)
//                                     Categorize.perform_training's model + criterion + optimizer (trex_learn_category.py:276-340) on the device: a
//                                     trexhip_trainer created from a 'TRXC' blob.  step(inputs, targets) is one pass of the loop body :317-334,
//                                     evaluate(inputs, targets) one batch of _predict_labels_and_loss (:356-373), export_blob() the weights as they
//                                     stand, load_into(categorize) hands them to the inference slot of a HipCategorize
// Define TREXHIP_CATEGORIZE_HOST_ONLY to leave out everything that calls the library (the host twin and sample_rows then need nothing but this file).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#ifndef TREXHIP_CATEGORIZE_HOST_ONLY
#include "../../include/trexhip.h"
#endif

namespace track {

struct CategoryVotes {
    int32_t n_tracklets = 0, categories = 0;
    std::vector<uint32_t> counts;      // [n_tracklets][categories]
    std::vector<uint32_t> rows;        // [n_tracklets]: every row handed in, skipped ones included
    std::vector<int32_t> label;        // [n_tracklets]: the first maximum of the counts, -1 when it is 0
    std::vector<float> share;          // [n_tracklets][categories]: counts / float(rows), 0 for an empty tracklet
    uint32_t skipped = 0;              // rows whose label was >= categories
};

struct CategorySampleRows {
    std::vector<int32_t> rows;         // indices into the tracklet's basic_index
    bool valid = false;                // false: Sample::Invalid() (fewer than min_samples rows)
};

// DataStore::temporary, CategorizeDatastore.cpp:1103-1152
inline CategorySampleRows category_sample_rows(size_t size, long first_frame, size_t sample_rate, size_t min_samples) {
    CategorySampleRows out;
    const size_t step = size < min_samples ? size_t(1) : std::max(size_t(1), sample_rate ? size / sample_rate : size);       // :1103
    long start_offset = 0;                                                                                                    // :1109-1113
    if (size >= 15u) {
        start_offset = first_frame;
        start_offset = 5 - start_offset % 5;
    }
    for (size_t i = 0; i + (size_t)start_offset < size; i += step) out.rows.push_back((int32_t)(i + (size_t)start_offset));  // :1117
    out.valid = out.rows.size() >= min_samples;                                                                               // :1145
    return out;
}

// CategorizeDatastore.cpp:555-585 and CategorizeInterface.cpp:212-247 on the host.  A tracklet id outside [0, n_tracklets) throws.
inline CategoryVotes category_label_averaged_host(const std::vector<int32_t>& labels, const std::vector<int32_t>& tracklet, int32_t n_tracklets, int32_t categories) {
    if (labels.size() != tracklet.size()) throw std::invalid_argument("label_averaged: one tracklet id per label");
    if (n_tracklets < 1 || categories < 1) throw std::invalid_argument("label_averaged: n_tracklets and categories must be positive");
    for (const int32_t t : tracklet)
        if (t < 0 || t >= n_tracklets) throw std::invalid_argument("label_averaged: a tracklet id was outside 0..n_tracklets-1");
    CategoryVotes v;
    v.n_tracklets = n_tracklets; v.categories = categories;
    const size_t T = (size_t)n_tracklets, C = (size_t)categories;
    v.counts.assign(T * C, 0u); v.rows.assign(T, 0u); v.label.assign(T, -1); v.share.assign(T * C, 0.f);
    for (size_t i = 0; i < labels.size(); ++i) {
        const size_t t = (size_t)tracklet[i];
        ++v.rows[t];                                                  // S = task.result.size()
        const int32_t l = labels[i];
        if (l < 0) continue;                                          // no label
        if ((size_t)l >= C) { ++v.skipped; continue; }                // "Label index > counts.size()": warned about, skipped
        ++v.counts[t * C + (size_t)l];
    }
    for (size_t t = 0; t < T; ++t) {
        const auto begin = v.counts.begin() + (std::ptrdiff_t)(t * C);
        const auto mit = std::max_element(begin, begin + (std::ptrdiff_t)C);
        if (*mit != 0) v.label[t] = (int32_t)(mit - begin);           // `if(*mit == 0) return nullptr`
        if (v.rows[t]) {
            const float S = (float)v.rows[t];
            for (size_t c = 0; c < C; ++c) v.share[t * C + c] = (float)v.counts[t * C + c] / S;
        }
    }
    return v;
}

#ifndef TREXHIP_CATEGORIZE_HOST_ONLY
struct HipCategorize {
    explicit HipCategorize(trexhip_ctx* ctx) : _ctx(ctx) { if (!ctx) throw std::invalid_argument("HipCategorize: null context"); }

    static void check(int rc) { if (rc != 0) throw std::runtime_error(std::string("libtrexhip: ") + trexhip_last_error()); }

    void load_weights(const void* blob, size_t bytes) { check(trexhip_categorize_load_weights(_ctx, blob, bytes)); }
    bool weights_loaded() const { return categories() > 0; }
    int32_t categories() const { int32_t c = 0; check(trexhip_categorize_info(_ctx, &c, nullptr, nullptr, nullptr)); return c; }

    // images: anything with data() (uint8, the network's H x W x C bytes) and size(); pointers (Image::Ptr) or values
    template <typename ImagePtr>
    std::vector<float> predict(const std::vector<ImagePtr>& images) const {
        int32_t cats = 0, ch = 0, W = 0, H = 0;
        check(trexhip_categorize_info(_ctx, &cats, &ch, &W, &H));
        if (!cats) throw std::runtime_error("Categorize: no weights loaded.");
        if (images.empty()) return {};                                 // `if len(images) == 0: return []`
        const size_t per = (size_t)W * H * ch;
        std::vector<uint8_t> crops;
        crops.reserve(images.size() * per);
        for (const auto& im : images) {
            if (!im || im->size() != per) throw std::runtime_error("Invalid image (expected individual_image_size and the category network's channels)");
            crops.insert(crops.end(), im->data(), im->data() + per);
        }
        std::vector<int32_t> labels(images.size());
        check(trexhip_categorize(_ctx, crops.data(), (int32_t)images.size(), labels.data()));
        return std::vector<float>(labels.begin(), labels.end());
    }

    // categories: of the loaded network when 0
    CategoryVotes label_averaged(const std::vector<int32_t>& labels, const std::vector<int32_t>& tracklet, int32_t n_tracklets, int32_t cats = 0) const {
        if (labels.size() != tracklet.size()) throw std::invalid_argument("label_averaged: one tracklet id per label");
        if (!cats) cats = categories();
        CategoryVotes v;
        v.n_tracklets = n_tracklets; v.categories = cats;
        const size_t T = (size_t)std::max(n_tracklets, 0), C = (size_t)std::max(cats, 0), n = labels.size();
        v.counts.assign(T * C, 0u); v.rows.assign(T, 0u); v.label.assign(T, -1); v.share.assign(T * C, 0.f);
        if (n == 0) return v;
        void* d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        struct Free { trexhip_ctx* c; void** p; ~Free() { for (int i = 0; i < 6; ++i) trexhip_device_free(c, p[i]); } } guard{_ctx, d};
        const size_t bytes[6] = {n * 4, n * 4, T * C * 4, T * 4, T * 4, T * C * 4};
        for (int i = 0; i < 6; ++i) check(trexhip_device_alloc(_ctx, bytes[i], &d[i]));
        check(trexhip_copy_to_device(_ctx, d[0], labels.data(), n * 4));
        check(trexhip_copy_to_device(_ctx, d[1], tracklet.data(), n * 4));
        check(trexhip_tracklet_labels_device(_ctx, static_cast<const int32_t*>(d[0]), static_cast<const int32_t*>(d[1]), (int32_t)n, n_tracklets, cats,
                                             static_cast<uint32_t*>(d[2]), static_cast<uint32_t*>(d[3]), static_cast<int32_t*>(d[4]), static_cast<float*>(d[5]),
                                             &v.skipped));
        check(trexhip_copy_to_host(_ctx, v.counts.data(), d[2], bytes[2]));
        check(trexhip_copy_to_host(_ctx, v.rows.data(), d[3], bytes[3]));
        check(trexhip_copy_to_host(_ctx, v.label.data(), d[4], bytes[4]));
        check(trexhip_copy_to_host(_ctx, v.share.data(), d[5], bytes[5]));
        return v;
    }

    static CategoryVotes label_averaged_host(const std::vector<int32_t>& labels, const std::vector<int32_t>& tracklet, int32_t n_tracklets, int32_t cats) {
        return category_label_averaged_host(labels, tracklet, n_tracklets, cats);
    }
    static CategorySampleRows sample_rows(size_t size, long first_frame, size_t sample_rate, size_t min_samples) {
        return category_sample_rows(size, first_frame, sample_rate, min_samples);
    }

    struct StepResult { float loss = 0.f; int32_t correct = 0; };

    // inputs: float32 [n][H][W][channels] in [0, 255] on the host (the crops as stored: the normalisation is the network's first layer);
    // targets: [n] category indices.  The dropout masks are the library's own draw
    struct Trainer {
        Trainer(trexhip_ctx* ctx, const void* blob, size_t bytes, int32_t max_batch = 32, float lr = 1e-4f, uint64_t seed = 0) {
            if (!ctx) throw std::invalid_argument("HipCategorize::Trainer: null context");
            trexhip_train_params p{};
            p.max_batch = max_batch; p.lr = lr; p.beta1 = 0.9f; p.beta2 = 0.999f; p.eps = 1e-8f; p.bn_momentum = 0.1f; p.dropout = 0.25f; p.precision = 1; p.seed = seed;
            check(trexhip_trainer_create(ctx, blob, bytes, &p, &_t));
            int32_t version = 0;
            check(trexhip_trainer_version(_t, &version));
            if (version != TREXHIP_NET_CATEGORY) { trexhip_trainer_destroy(_t); throw std::invalid_argument("HipCategorize::Trainer: not a category blob ('TRXC')"); }
            _bytes = bytes;
            int32_t hdr[8];
            std::memcpy(hdr, blob, sizeof(hdr));                        // (the library has accepted the blob: it holds its header)
            _channels = hdr[5];
            check(trexhip_trainer_image_size(_t, &_width, &_height));
        }
        ~Trainer() { trexhip_trainer_destroy(_t); }
        Trainer(const Trainer&) = delete;
        Trainer& operator=(const Trainer&) = delete;

        StepResult step(const std::vector<float>& inputs, const std::vector<int32_t>& targets) {
            StepResult r;
            check_batch(inputs, targets);
            check(trexhip_train_step(_t, inputs.data(), targets.data(), (int32_t)targets.size(), nullptr, &r.loss, &r.correct));
            return r;
        }
        StepResult evaluate(const std::vector<float>& inputs, const std::vector<int32_t>& targets) {
            StepResult r;
            check_batch(inputs, targets);
            check(trexhip_train_eval(_t, inputs.data(), targets.data(), (int32_t)targets.size(), &r.loss, &r.correct));
            return r;
        }
        int64_t steps() const { return trexhip_trainer_steps(_t); }
        std::vector<uint8_t> export_blob() {
            std::vector<uint8_t> blob(_bytes);
            size_t got = 0;
            check(trexhip_trainer_export(_t, blob.data(), blob.size(), &got));
            return blob;
        }
        void load_into(HipCategorize& categorize) {
            const std::vector<uint8_t> blob = export_blob();
            categorize.load_weights(blob.data(), blob.size());
        }
        trexhip_trainer* handle() const { return _t; }

      private:
        void check_batch(const std::vector<float>& inputs, const std::vector<int32_t>& targets) const {
            if (targets.empty() || inputs.size() != targets.size() * (size_t)_width * _height * _channels)
                throw std::invalid_argument("HipCategorize::Trainer: inputs must be [n][H][W][channels] for n targets");
        }
        trexhip_trainer* _t = nullptr;
        size_t _bytes = 0;
        int32_t _width = 0, _height = 0, _channels = 0;
    };

  private:
    trexhip_ctx* _ctx;
};
#endif

}  // namespace track
