// test_host_tracklet_images.cpp -- track::tracklet_images_device (trex_amd/host/HipTrackletImages.h) against its host twin, the loop of
// Application/src/tracker/ui/Export.cpp:1287-1364 with hist_utils::addImage (:78-154) line for line: byte for byte, in the reference's
// output order (by individual id, then by range), keeping only tracklets of more than one image (:1355).
// usage: test_host_tracklet_images            (needs a GPU)
//        test_host_tracklet_images --host     (the host twin alone, against sorted stacks)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../trex_amd/host/HipTrackletImages.h"

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

using track::Idx_t;
using cmn::Frame_t;
using FrameRange = cmn::Range<Frame_t>;
using Rows = track::TrackletRows<Idx_t, FrameRange>;

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 24; }

// three individuals with tracklets of 1, 2 and 5 images each, given out of order and with their pool rows interleaved; rows 0 and 13 are in no tracklet
static std::vector<Rows> grouping() {
    auto range = [](int a, int b) { return FrameRange(Frame_t(a), Frame_t(b)); };
    std::vector<Rows> t;
    t.push_back({Idx_t(2), range(40, 44), {3, 9, 14, 20, 25}});
    t.push_back({Idx_t(0), range(10, 11), {4, 1}});
    t.push_back({Idx_t(1), range(0, 0), {2}});
    t.push_back({Idx_t(0), range(0, 4), {5, 10, 15, 21, 24}});
    t.push_back({Idx_t(2), range(0, 0), {6}});
    t.push_back({Idx_t(1), range(30, 34), {7, 11, 16, 19, 23}});
    t.push_back({Idx_t(0), range(5, 5), {8}});
    t.push_back({Idx_t(1), range(10, 11), {12, 17}});
    t.push_back({Idx_t(2), range(10, 11), {18, 22}});
    return t;
}
static const int32_t WANT_META[][3] = {{0, 0, 4}, {0, 10, 11}, {1, 10, 11}, {1, 30, 34}, {2, 10, 11}, {2, 40, 44}};
static const size_t POOL = 26;

static int check_against_sorted(const std::vector<uint8_t>& pool, int W, int H, int C, const std::vector<Rows>& groups, const track::TrackletImages& got) {
    const size_t px = (size_t)W * H, per = px * C;
    REQUIRE(got.all_ranges.size() == 6 * 3 && got.all_images.size() == 6 * px);
    for (size_t k = 0; k < 6; ++k) {
        REQUIRE(std::memcmp(&got.all_ranges[3 * k], WANT_META[k], sizeof(WANT_META[k])) == 0);
        const Rows* mine = nullptr;
        for (const auto& g : groups)
            if ((int32_t)g.id.get() == WANT_META[k][0] && g.range.start.get() == WANT_META[k][1] && g.range.end.get() == WANT_META[k][2]) mine = &g;
        REQUIRE(mine);
        for (size_t i = 0; i < px; ++i) {
            std::vector<uint8_t> v;
            for (int32_t r : mine->rows) {
                const uint8_t* p = &pool[(size_t)r * per + i * C];
                v.push_back(C == 1 ? p[0] : (uint8_t)((p[0] * 1868u + p[1] * 9617u + p[2] * 4899u + 8192u) >> 14));
            }
            std::sort(v.begin(), v.end());
            REQUIRE(got.all_images[k * px + i] == v[v.size() / 2]);     // the upper median at an even count
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    const bool host_only = argc > 1 && std::strcmp(argv[1], "--host") == 0;
    const auto groups = grouping();
    try {
        trexhip_ctx* ctx = nullptr;
        if (!host_only) {
            trexhip_params p;
            trexhip_default_params(&p, 64, 64);
            p.max_batch = 1;
            REQUIRE(trexhip_create(&p, &ctx) == 0);
        }
        struct Destroy { trexhip_ctx*& c; ~Destroy() { if (c) trexhip_destroy(c); } } destroy{ctx};
        const int shapes[][3] = {{80, 80, 1}, {13, 11, 3}, {9, 8, 1}};   // W, H, C
        for (const auto& s : shapes) {
            const int W = s[0], H = s[1], C = s[2];
            const size_t per = (size_t)W * H * C;
            std::vector<uint8_t> pool(POOL * per);
            uint32_t seed = 7u + (uint32_t)per;
            for (auto& b : pool) b = (uint8_t)lcg(seed);
            for (size_t i = 0; i < per; ++i) pool[0 * per + i] = pool[13 * per + i] = 255;      // the rows of no tracklet would show
            const auto host = track::tracklet_images_host(pool.data(), POOL, W, H, C, groups);
            if (int rc = check_against_sorted(pool, W, H, C, groups, host)) return rc;
            if (host_only) continue;
            void* d_pool = nullptr;
            REQUIRE(trexhip_device_alloc(ctx, pool.size(), &d_pool) == 0);
            REQUIRE(trexhip_copy_to_device(ctx, d_pool, pool.data(), pool.size()) == 0);
            const auto dev = track::tracklet_images_device(ctx, d_pool, POOL, W, H, C, groups);
            REQUIRE(dev.all_ranges == host.all_ranges);
            REQUIRE(dev.all_images == host.all_images);
            // the order in which the caller lists the tracklets does not matter
            auto reversed = groups;
            std::reverse(reversed.begin(), reversed.end());
            const auto dev2 = track::tracklet_images_device(ctx, d_pool, POOL, W, H, C, reversed);
            REQUIRE(dev2.all_ranges == host.all_ranges && dev2.all_images == host.all_images);
            // nothing but single images: nothing is kept
            std::vector<Rows> singles = {groups[2], groups[4], groups[6]};
            const auto none = track::tracklet_images_device(ctx, d_pool, POOL, W, H, C, singles);
            REQUIRE(none.all_images.empty() && none.all_ranges.empty());
            REQUIRE(track::tracklet_images_device(ctx, d_pool, POOL, W, H, C, std::vector<Rows>{}).all_images.empty());
            REQUIRE(trexhip_device_free(ctx, d_pool) == 0);
        }
        {   // refused alike by both routes, before anything runs: a row listed twice, a row outside the pool, two channels
            std::vector<uint8_t> pool(POOL * 64);
            auto twice = groups;
            twice[0].rows[0] = 4;
            auto outside = groups;
            outside[1].rows[1] = (int32_t)POOL;
            int threw = 0;
            try { track::tracklet_images_host(pool.data(), POOL, 8, 8, 1, twice); } catch (const std::invalid_argument&) { ++threw; }
            try { track::tracklet_images_host(pool.data(), POOL, 8, 8, 1, outside); } catch (const std::invalid_argument&) { ++threw; }
            try { track::tracklet_images_host(pool.data(), POOL, 8, 8, 2, groups); } catch (const std::invalid_argument&) { ++threw; }
            try { track::tracklet_images_device(ctx, nullptr, POOL, 8, 8, 1, twice); } catch (const std::invalid_argument&) { ++threw; }
            try { track::tracklet_images_device(ctx, nullptr, POOL, 8, 8, 2, groups); } catch (const std::invalid_argument&) { ++threw; }
            REQUIRE(threw == 5);
        }
        std::printf("tracklet images adapter ok: %s, 9 tracklets of 3 individuals -> 6 medians at 3 sizes\n", host_only ? "host twin" : "device route = host twin");
    } catch (const std::exception& e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    return 0;
}
