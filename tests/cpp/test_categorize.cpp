// test_categorize.cpp -- trex_amd/host/HipCategorize.h.
//   host mode (built with -DTREXHIP_CATEGORIZE_HOST_ONLY, plain g++, no library):  test_categorize vectors.bin
//       the host twin of the vote and sample_rows against vectors written by the Python restatement (tests/category_ref.py), byte for byte
//   device mode (linked against libtrexhip):  test_categorize vectors.bin blob.bin crops.bin labels.bin
//       predict on the category network against the labels the Python wrapper got, and label_averaged on the device = its host twin
// vectors.bin: int32 votes, per vote {int32 n, T, C; int32 labels[n], tracklet[n]; uint32 counts[T*C], rows[T]; int32 label[T]; float share[T*C];
// uint32 skipped}; int32 samples, per sample {int64 size, first_frame, sample_rate, min_samples; int32 count, valid; int32 rows[count]}
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>
#include "../../trex_amd/host/HipCategorize.h"

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

struct Reader {
    const std::vector<char>& b;
    size_t at = 0;
    bool ok = true;
    template <class T> T one() { T v{}; if (at + sizeof(T) > b.size()) { ok = false; return v; } std::memcpy(&v, b.data() + at, sizeof(T)); at += sizeof(T); return v; }
    template <class T> std::vector<T> many(size_t n) {
        std::vector<T> v(n);
        if (at + n * sizeof(T) > b.size()) { ok = false; return v; }
        if (n) std::memcpy(v.data(), b.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Crop {      // the surface predict() needs of an image
    std::vector<uint8_t> px;
    const uint8_t* data() const { return px.data(); }
    size_t size() const { return px.size(); }
};

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s vectors.bin [blob.bin crops.bin labels.bin]\n", argv[0]); return 2; }
    const auto vec = slurp(argv[1]);
    Reader r{vec};
    const int32_t votes = r.one<int32_t>();
    REQUIRE(r.ok && votes > 0);
#ifndef TREXHIP_CATEGORIZE_HOST_ONLY
    REQUIRE(argc >= 5);
    trexhip_params p;
    trexhip_default_params(&p, 64, 64);
    trexhip_ctx* ctx = nullptr;
    REQUIRE(trexhip_create(&p, &ctx) == 0);
    struct Destroy { trexhip_ctx* c; ~Destroy() { trexhip_destroy(c); } } destroy{ctx};
#endif
    try {
        for (int32_t k = 0; k < votes; ++k) {
            const int32_t n = r.one<int32_t>(), T = r.one<int32_t>(), C = r.one<int32_t>();
            REQUIRE(r.ok && n >= 0 && T > 0 && C > 0);
            const auto labels = r.many<int32_t>((size_t)n), tracklet = r.many<int32_t>((size_t)n);
            const auto counts = r.many<uint32_t>((size_t)T * C), rows = r.many<uint32_t>((size_t)T);
            const auto label = r.many<int32_t>((size_t)T);
            const auto share = r.many<float>((size_t)T * C);
            const uint32_t skipped = r.one<uint32_t>();
            REQUIRE(r.ok);
            const track::CategoryVotes h = track::category_label_averaged_host(labels, tracklet, T, C);
            REQUIRE(same(h.counts, counts) && same(h.rows, rows) && same(h.label, label) && same(h.share, share) && h.skipped == skipped);
#ifndef TREXHIP_CATEGORIZE_HOST_ONLY
            const track::CategoryVotes d = track::HipCategorize(ctx).label_averaged(labels, tracklet, T, C);
            REQUIRE(same(d.counts, h.counts) && same(d.rows, h.rows) && same(d.label, h.label) && same(d.share, h.share) && d.skipped == h.skipped);
#endif
        }
        const int32_t samples = r.one<int32_t>();
        REQUIRE(r.ok && samples > 0);
        for (int32_t k = 0; k < samples; ++k) {
            const int64_t size = r.one<int64_t>(), first = r.one<int64_t>(), rate = r.one<int64_t>(), min_samples = r.one<int64_t>();
            const int32_t count = r.one<int32_t>(), valid = r.one<int32_t>();
            const auto rows = r.many<int32_t>((size_t)count);
            REQUIRE(r.ok);
            const track::CategorySampleRows s = track::category_sample_rows((size_t)size, (long)first, (size_t)rate, (size_t)min_samples);
            REQUIRE(same(s.rows, rows) && (int32_t)s.valid == valid);
        }
        REQUIRE(r.at == vec.size());
        bool threw = false;
        try { track::category_label_averaged_host({0, 1}, {0, 2}, 2, 2); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
#ifndef TREXHIP_CATEGORIZE_HOST_ONLY
        const auto blob = slurp(argv[2]), crops = slurp(argv[3]), want = slurp(argv[4]);
        track::HipCategorize cat(ctx);
        REQUIRE(!cat.weights_loaded());
        threw = false;
        try { cat.predict(std::vector<std::unique_ptr<Crop>>{}); } catch (const std::runtime_error&) { threw = true; }
        REQUIRE(threw);                                               // no weights
        cat.load_weights(blob.data(), blob.size());
        int32_t cats = 0, ch = 0, W = 0, H = 0;
        REQUIRE(trexhip_categorize_info(ctx, &cats, &ch, &W, &H) == 0 && cat.categories() == cats && cats > 0);
        const size_t per = (size_t)W * H * ch, n = crops.size() / per;
        REQUIRE(n > 0 && want.size() == n * 4);
        std::vector<std::unique_ptr<Crop>> images;
        for (size_t i = 0; i < n; ++i) {
            images.push_back(std::make_unique<Crop>());
            images.back()->px.assign(reinterpret_cast<const uint8_t*>(crops.data()) + i * per, reinterpret_cast<const uint8_t*>(crops.data()) + (i + 1) * per);
        }
        const std::vector<float> got = cat.predict(images);
        REQUIRE(got.size() == n);
        for (size_t i = 0; i < n; ++i) {
            int32_t w;
            std::memcpy(&w, want.data() + 4 * i, 4);
            REQUIRE(got[i] == (float)w);
        }
        REQUIRE(cat.predict(std::vector<std::unique_ptr<Crop>>{}).empty());
        // the labels as tracklets of three rows each, voted on the device with the network's own category count
        std::vector<int32_t> lab(got.begin(), got.end()), tr(n);
        for (size_t i = 0; i < n; ++i) tr[i] = (int32_t)(i / 3);
        const int32_t T = (int32_t)((n + 2) / 3);
        const track::CategoryVotes d = cat.label_averaged(lab, tr, T), h = track::HipCategorize::label_averaged_host(lab, tr, T, cats);
        REQUIRE(same(d.counts, h.counts) && same(d.rows, h.rows) && same(d.label, h.label) && same(d.share, h.share) && d.skipped == 0 && h.skipped == 0);
        std::printf("categorize adapter ok: %d votes, %d samples, %zu crops\n", votes, samples, n);
#else
        std::printf("categorize host twin ok: %d votes, %d samples\n", votes, samples);
#endif
    } catch (const std::exception& e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
