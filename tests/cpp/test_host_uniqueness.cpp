// test_host_uniqueness.cpp -- track::calculate_uniqueness (trex_amd/host/HipUniqueness.h) against the reference's loop
// (Application/src/tracker/ui/Accumulation.cpp:799-878) run here on the probabilities the same network hands to the host.
// usage: test_host_uniqueness weights.bin crops.bin   (crops: uint8 [n][80][80][1], n >= 40)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <map>
#include <vector>
#include "../../trex_amd/host/HipUniqueness.h"

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: %s weights.bin crops.bin\n", argv[0]); return 2; }
    const auto blob = slurp(argv[1]);
    const auto crops = slurp(argv[2]);
    const size_t per = 80 * 80, n = crops.size() / per;
    REQUIRE(n >= 40);
    try {
        track::HipVINetwork net(0);
        net.load_weights(blob.data(), blob.size());
        const size_t N = (size_t)net.num_classes();
        auto images = [&]() {
            std::vector<cmn::Image::Ptr> v;
            for (size_t i = 0; i < n; ++i) {
                auto im = cmn::Image::Make(80, 80, 1);
                std::copy(crops.begin() + i * per, crops.begin() + (i + 1) * per, reinterpret_cast<char*>(im->data()));
                v.push_back(std::move(im));
            }
            return v;
        };
        // frames of different lengths, one empty, two that overlap, a gap behind the last
        std::map<cmn::Frame_t, cmn::Range<size_t>> map_indexes;
        map_indexes[cmn::Frame_t(10)] = {0, 8};
        map_indexes[cmn::Frame_t(11)] = {8, 8};
        map_indexes[cmn::Frame_t(12)] = {6, 25};
        map_indexes[cmn::Frame_t(20)] = {25, 26};
        map_indexes[cmn::Frame_t(21)] = {26, n - 3};
        std::vector<float> per_class;
        const auto imgs = images();
        const auto [ratio, unique_percent, mean] = track::calculate_uniqueness(net, imgs, map_indexes, &per_class);

        // the reference's loop on the host's copy of the same probabilities
        const std::vector<float> predictions = net.probabilities(images());
        REQUIRE(predictions.size() == n * N && per_class.size() == N);
        size_t good_frames = 0, bad_frames = 0;
        double percentages = 0;
        double worst = 0;
        std::vector<float> id_sum(N, 0.f), id_count(N, 0.f);
        for (const auto& [frame, range] : map_indexes) {
            std::map<size_t, float> probs;
            for (size_t i = range.start; i < range.end; ++i) {
                long max_id = -1;
                float max_p = 0;
                for (size_t id = 0; id < N; ++id) {
                    const float p = predictions.at(i * N + id);
                    if (p > max_p) { max_p = p; max_id = (long)id; }
                }
                if (max_id >= 0) probs[(size_t)max_id] = std::max(probs[(size_t)max_id], max_p);
            }
            double p = range.length() <= 0 ? 0 : (probs.size() / float(range.length()));
            float accum_p = 0;
            for (const auto& [id, pp] : probs) { accum_p += pp; id_sum[id] += pp; ++id_count[id]; }
            static const float NORMAL = (1 + expf(-1 * float(M_PI) * 1));
            if (!probs.empty()) p = 1 / (1 + exp(-(accum_p / float(probs.size())) * M_PI * 1)) * NORMAL * p;
            percentages += p;
            if (probs.size() == range.length()) ++good_frames; else ++bad_frames;
            REQUIRE(unique_percent.count(frame) == 1);
            worst = std::max(worst, std::fabs((double)unique_percent.at(frame) - (double)float(p)));
        }
        REQUIRE(unique_percent.size() == map_indexes.size());
        REQUIRE(worst <= 2.4e-7);
        REQUIRE(ratio == float(good_frames) / float(good_frames + bad_frames));
        const float want_mean = float(percentages / double(map_indexes.size()));
        REQUIRE(std::fabs(mean - want_mean) <= std::nextafter(std::fabs(want_mean), 2.f) - std::fabs(want_mean));
        REQUIRE(unique_percent.at(cmn::Frame_t(11)) == 0.f);
        for (size_t id = 0; id < N; ++id) {
            const float want = id_count[id] > 0 ? id_sum[id] / id_count[id] : 0.f;
            REQUIRE(std::fabs(per_class[id] - want) <= id_count[id] * std::ldexp(1.0, -24) * want);
        }
        std::printf("uniqueness adapter ok: %zu crops, %zu classes, %zu good / %zu bad frames, mean %.6f, max |d unique_percent| = %.3g\n", n, N, good_frames,
                    bad_frames, (double)mean, worst);
    } catch (const std::exception& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
