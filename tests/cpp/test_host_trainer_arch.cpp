// test_host_trainer_arch.cpp -- HipVINetwork::Trainer (trex_amd/host/HipVINetwork.h) on a v100 blob: train_batch, evaluate, and weights() round
// tripping through HipVINetwork::load_weights into the inference chain.
// usage: test_host_trainer_arch weights.bin crops.bin W H classes   (weights: a v100 blob at W x H x 1; crops: uint8 [n][H][W][1], n >= 8)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>
#include "../../trex_amd/host/HipVINetwork.h"

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 6) { std::printf("usage: %s weights.bin crops.bin W H classes\n", argv[0]); return 2; }
    const auto blob = slurp(argv[1]);
    const auto crops = slurp(argv[2]);
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), C = std::atoi(argv[5]);
    const size_t per = (size_t)W * H, n = crops.size() / per;
    REQUIRE(n >= 8 && n <= 64);
    try {
        track::HipVINetwork net(0);
        track::HipVINetwork::Trainer tr(net, blob.data(), blob.size(), 64, 1e-5f, 7);
        REQUIRE(tr.version() == TREXHIP_NET_V100);
        std::vector<float> x(n * per);
        std::vector<int32_t> y(n);
        for (size_t i = 0; i < x.size(); ++i) x[i] = (float)(unsigned char)crops[i];
        for (size_t i = 0; i < n; ++i) y[i] = (int32_t)(i % (size_t)C);
        const auto before = tr.evaluate(x.data(), y.data(), (int)n);
        REQUIRE(std::isfinite(before.loss) && before.correct >= 0 && before.correct <= (int)n && tr.steps() == 0);
        auto last = tr.train_batch(x.data(), y.data(), (int)n);
        for (int k = 0; k < 2; ++k) last = tr.train_batch(x.data(), y.data(), (int)n);
        REQUIRE(std::isfinite(last.loss) && last.correct >= 0 && last.correct <= (int)n && tr.steps() == 3);
        y[0] = C;                                                                       // label out of range: refused
        bool threw = false; try { tr.train_batch(x.data(), y.data(), (int)n); } catch (const std::exception&) { threw = true; } REQUIRE(threw);
        y[0] = 0;
        REQUIRE(tr.steps() == 3);
        const auto val = tr.evaluate(x.data(), y.data(), (int)n);                       // eval mode: nothing dropped, nothing changes
        REQUIRE(std::isfinite(val.loss) && tr.steps() == 3);
        const auto w = tr.weights();
        int32_t id = -1;
        std::memcpy(&id, w.data() + 24, 4);
        REQUIRE(w.size() == blob.size() && id == TREXHIP_NET_V100 && std::memcmp(w.data(), blob.data(), 32) == 0 && std::memcmp(w.data(), blob.data(), w.size()) != 0);
        // the round trip: the inference chain on the exported weights counts what the trainer's own evaluation counted
        tr.apply();
        REQUIRE(net.num_classes() == C);
        std::vector<cmn::Image::Ptr> images;
        for (size_t i = 0; i < n; ++i) {
            auto im = cmn::Image::Make(H, W, 1);
            std::copy(crops.begin() + i * per, crops.begin() + (i + 1) * per, reinterpret_cast<char*>(im->data()));
            images.push_back(std::move(im));
        }
        const std::vector<float> p = net.probabilities(std::move(images));
        REQUIRE(p.size() == n * (size_t)C);
        int correct = 0;
        for (size_t i = 0; i < n; ++i) {
            int best = 0;
            float sum = 0.f;
            for (int c = 0; c < C; ++c) { sum += p[i * C + c]; if (p[i * C + c] > p[i * C + best]) best = c; }
            REQUIRE(std::fabs(sum - 1.f) <= 1e-4f);
            correct += best == y[i];
        }
        REQUIRE(correct == val.correct);
        std::printf("v100 trainer facade ok: loss %.4f -> %.4f in 3 steps, %d of %zu correct on both chains\n", before.loss, val.loss, correct, n);
    } catch (const std::exception& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
