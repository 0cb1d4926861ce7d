// test_categorize_trainer.cpp -- HipCategorize::Trainer (trex_amd/host/HipCategorize.h) through the C ABI:
//   test_categorize_trainer blob.bin x.bin y.bin crops.bin out.bin
// blob.bin: a 'TRXC' blob; x.bin: float32 [n][H][W][C]; y.bin: int32 [n]; crops.bin: uint8 [m][H][W][C].  Three steps, an evaluation, the export, and
// load_into a HipCategorize whose predict then labels the crops.  out.bin: float32 loss[3], int32 correct[3], float32 eval loss, int32 eval correct,
// int32 labels[m], then the exported blob -- the Python side (tests/test_categorize_trainer_cpp_gpu.py) holds them to the Python wrapper's own run.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "../../trex_amd/host/HipCategorize.h"

static std::vector<char> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main(int argc, char** argv) {
    REQUIRE(argc == 6);
    const std::vector<char> blob = slurp(argv[1]), xb = slurp(argv[2]), yb = slurp(argv[3]), cb = slurp(argv[4]);
    REQUIRE(blob.size() >= 32 && !yb.empty() && yb.size() % 4 == 0 && xb.size() % 4 == 0);
    int32_t hdr[8];
    std::memcpy(hdr, blob.data(), 32);
    const size_t per = (size_t)hdr[3] * hdr[4] * hdr[5], n = yb.size() / 4;
    REQUIRE(xb.size() == n * per * 4 && cb.size() % per == 0);
    std::vector<float> x(n * per);
    std::vector<int32_t> y(n);
    std::memcpy(x.data(), xb.data(), xb.size());
    std::memcpy(y.data(), yb.data(), yb.size());
    trexhip_params p;
    trexhip_default_params(&p, 64, 64);
    trexhip_ctx* ctx = nullptr;
    REQUIRE(trexhip_create(&p, &ctx) == 0);
    struct Destroy { trexhip_ctx* c; ~Destroy() { trexhip_destroy(c); } } destroy{ctx};
    try {
        std::ofstream out(argv[5], std::ios::binary);
        track::HipCategorize cat(ctx);
        REQUIRE(!cat.weights_loaded());
        {
            track::HipCategorize::Trainer trainer(ctx, blob.data(), blob.size(), (int32_t)n, 1e-4f, 5);
            float loss[3];
            int32_t correct[3];
            for (int s = 0; s < 3; ++s) {
                const track::HipCategorize::StepResult r = trainer.step(x, y);
                loss[s] = r.loss; correct[s] = r.correct;
            }
            REQUIRE(trainer.steps() == 3);
            const track::HipCategorize::StepResult e = trainer.evaluate(x, y);
            out.write(reinterpret_cast<const char*>(loss), sizeof(loss));
            out.write(reinterpret_cast<const char*>(correct), sizeof(correct));
            out.write(reinterpret_cast<const char*>(&e.loss), 4);
            out.write(reinterpret_cast<const char*>(&e.correct), 4);
            bool threw = false;
            try { trainer.step(std::vector<float>(per - 1), std::vector<int32_t>(1, 0)); } catch (const std::invalid_argument&) { threw = true; }
            REQUIRE(threw);
            trainer.load_into(cat);
            REQUIRE(cat.categories() == hdr[2]);
            std::vector<std::vector<uint8_t>> images;
            for (size_t i = 0; i < cb.size() / per; ++i) images.emplace_back(cb.begin() + (std::ptrdiff_t)(i * per), cb.begin() + (std::ptrdiff_t)((i + 1) * per));
            std::vector<const std::vector<uint8_t>*> ptrs;
            for (const auto& im : images) ptrs.push_back(&im);
            const std::vector<float> labels = cat.predict(ptrs);
            std::vector<int32_t> li(labels.begin(), labels.end());
            out.write(reinterpret_cast<const char*>(li.data()), (std::streamsize)(li.size() * 4));
            const std::vector<uint8_t> exported = trainer.export_blob();
            REQUIRE(exported.size() == blob.size());
            out.write(reinterpret_cast<const char*>(exported.data()), (std::streamsize)exported.size());
        }
        bool refused = false;                                            // an identity blob is not a category trainer
        try {
            std::vector<char> ident = blob;
            const int32_t magic = 0x57585254;                            // 'TRXW'
            std::memcpy(ident.data(), &magic, 4);
            track::HipCategorize::Trainer t2(ctx, ident.data(), ident.size());
        } catch (const std::exception&) { refused = true; }
        REQUIRE(refused);
        std::printf("categorize trainer ok: %zu samples, %zu crops\n", n, cb.size() / per);
    } catch (const std::exception& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
