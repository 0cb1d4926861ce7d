// test_host_accumulation.cpp -- track::paverages_device (trex_amd/host/HipAccumulation.h) against HipVINetwork::paverages, the host loop of
// VINetwork::paverages (Application/src/tracker/ml/VisualIdentification.h:145-180), on the same network and crops: bit for bit.  Then
// track::decide_additional_range on the result.
// usage: test_host_accumulation weights.bin crops.bin   (crops: uint8 [n][80][80][1], n >= 48)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <vector>
#include "../../trex_amd/host/HipAccumulation.h"

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
    REQUIRE(n >= 48);
    using track::Idx_t;
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
        // ids 0, 1, 2, 5, 6 (3 and 4 never occur: a gap), unevenly many rows each, not grouped; id 6 owns the last rows only
        std::vector<Idx_t> ids(n);
        const uint32_t pattern[] = {5, 0, 2, 0, 1, 5, 5, 0, 2, 0, 0};
        for (size_t i = 0; i < n; ++i) ids[i] = Idx_t(i + 3 >= n ? 6u : pattern[i % 11]);
        const auto imgs = images();
        const auto got = track::paverages_device(net, ids, imgs);
        const auto want = net.paverages(ids, images());
        REQUIRE(got.size() == 5 && want.size() == 5);
        auto g = got.begin();
        for (auto w = want.begin(); w != want.end(); ++w, ++g) {
            REQUIRE(g->first == w->first);
            REQUIRE(g->second.samples == w->second.samples);
            REQUIRE(g->second.values.size() == N && w->second.values.size() == N);
            REQUIRE(std::memcmp(g->second.values.data(), w->second.values.data(), N * sizeof(float)) == 0);
        }
        REQUIRE(got.count(Idx_t(3)) == 0 && got.count(Idx_t(4)) == 0 && got.at(Idx_t(6)).samples == 3.f);
        // fewer ids than images: the rows behind the last id are predicted and left out, as the reference's loop leaves them out
        std::vector<Idx_t> fewer(ids.begin(), ids.begin() + 20);
        const auto got20 = track::paverages_device(net, fewer, imgs);
        const auto want20 = net.paverages(fewer, images());
        REQUIRE(got20.size() == want20.size());
        for (const auto& kv : want20) {
            REQUIRE(got20.at(kv.first).samples == kv.second.samples);
            REQUIRE(std::memcmp(got20.at(kv.first).values.data(), kv.second.values.data(), N * sizeof(float)) == 0);
        }
        REQUIRE(track::paverages_device(net, std::vector<Idx_t>{}, imgs).empty());
        {   // an image of the wrong size is refused, as calculate_uniqueness refuses it
            std::vector<cmn::Image::Ptr> bad;
            bad.push_back(cmn::Image::Make(64, 64, 1));
            bool threw = false;
            try { track::paverages_device(net, std::vector<Idx_t>{Idx_t(0)}, bad); } catch (const std::exception&) { threw = true; }
            REQUIRE(threw);
        }
        const auto d = track::decide_additional_range(got, (uint32_t)N, 1.f);
        REQUIRE(d.max_indexes.size() == got.size());
        REQUIRE(d.status == track::RangeStatus::Acceptable || d.status == track::RangeStatus::NoUniqueIDs || d.status == track::RangeStatus::ProbabilityTooLow);
        for (const auto& kv : got) {
            float m = 0;
            for (float v : kv.second.values) m = v > m ? v : m;
            REQUIRE(d.min_prob <= m);
        }
        std::printf("accumulation adapter ok: %zu crops, %zu classes, %zu individuals, status %d, min_prob %.6f\n", n, N, got.size(), (int)d.status, (double)d.min_prob);
    } catch (const std::exception& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
