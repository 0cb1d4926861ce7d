// Drives track::HipPrefilter (trex_amd/host/HipPrefilter.h) through the C ABI on one hand-worked batch: 64 x 48 frames on a flat background
// of 200; frame 0 holds a 30-pixel blob (in range), a 4-pixel blob (below) and a 120-pixel blob (above), frame 1 a 30-pixel blob inside
// an ignore rectangle.  track_size_filter (20, 100), track_threshold 30.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../trex_amd/host/HipPrefilter.h"

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static void rect(std::vector<uint8_t>& f, int W, int x0, int y0, int x1, int y1, uint8_t v) {
    for (int y = y0; y <= y1; ++y) for (int x = x0; x <= x1; ++x) f[(size_t)y * W + x] = v;
}

int main(int argc, char** argv) {
    const int W = 64, H = 48, N = 2, MAX_BLOBS = 8;
    // packing is host code: checked without a device
    {
        std::vector<std::vector<cmn::Vec2>> shapes = {{{1, 2}, {3, 4}}, {{0, 0}, {5, 0}, {5, 5}}};
        auto t = track::HipPrefilter::pack_shapes(shapes);
        REQUIRE(t.offsets == (std::vector<int32_t>{0, 2, 5}) && t.points.size() == 10 && t.points[4] == 0.f && t.points[9] == 5.f);
        std::vector<uint32_t> words; std::vector<int32_t> off;
        track::HipPrefilter::pack_bdx({{9u, 3u}, {}}, 3, words, off);
        REQUIRE(words == (std::vector<uint32_t>{3u, 9u}) && off == (std::vector<int32_t>{0, 2, 2, 2}));
    }
    if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) { std::printf("prefilter packing ok\n"); return 0; }
    trexhip_params p;
    trexhip_default_params(&p, W, H);
    p.max_batch = N; p.max_blobs = MAX_BLOBS; p.cm_per_pixel = 1.0;
    trexhip_ctx* ctx = nullptr;
    REQUIRE(trexhip_create(&p, &ctx) == 0);
    std::vector<uint8_t> bg((size_t)W * H, 200), f0 = bg, f1 = bg;
    rect(f0, W, 4, 4, 9, 8, 100); rect(f0, W, 20, 4, 21, 5, 100); rect(f0, W, 30, 4, 41, 13, 100);
    rect(f1, W, 4, 30, 9, 34, 100);
    REQUIRE(trexhip_set_background(ctx, bg.data(), W) == 0);
    const uint8_t* frames[2] = {f0.data(), f1.data()};
    REQUIRE(trexhip_segment(ctx, frames, W, N) == 0);
    trexhip_batch_result det;
    REQUIRE(trexhip_fetch(ctx, &det) == 0);
    REQUIRE(det.total_blobs == 4);
    track::HipPrefilter::Settings st;
    st.track_threshold = 30;
    st.track_size_filter = {cmn::Range<double>(20, 100)};
    st.track_ignore = {{{0, 28}, {20, 40}}};
    trexhip_batch_result sub;
    auto r = track::HipPrefilter::apply(ctx, st, det, N, MAX_BLOBS, &sub);
    REQUIRE(r.frames.size() == 2 && !r.frames[0].undecided && !r.frames[1].undecided);
    const auto& a = r.frames[0];
    REQUIRE(a.filtered.size() == 1 && a.big.size() == 1 && a.filtered_out.size() == 1);
    REQUIRE(a.filtered[0].thresholded && sub.blobs[a.filtered[0].index].n_pixels == 30);
    REQUIRE(a.big[0].thresholded && sub.blobs[a.big[0].index].n_pixels == 120);
    REQUIRE(!a.filtered_out[0].entry.thresholded && det.blobs[a.filtered_out[0].entry.index].n_pixels == 4 &&
            a.filtered_out[0].reason == TREXHIP_FILTER_OUTSIDE_RANGE);
    const auto& b = r.frames[1];
    REQUIRE(b.filtered.empty() && b.big.empty() && b.filtered_out.size() == 1 && b.filtered_out[0].entry.thresholded &&
            b.filtered_out[0].reason == TREXHIP_FILTER_INSIDE_IGNORE);
    // presumed_nr: 2 for the parent of the big blob, else 0
    int twos = 0;
    for (uint32_t k = 0; k < det.total_blobs; ++k) {
        REQUIRE(r.presumed_nr[k] == (det.blobs[k].n_pixels == 120 ? 2 : 0));
        twos += r.presumed_nr[k] == 2;
    }
    REQUIRE(twos == 1);
    // the host twin of the policy on the two fetched table sets gives the same lists, with and without the second threshold
    for (int thr2 : {0, 60}) {
        st.track_threshold_2 = thr2;
        st.threshold_ratio_range = cmn::Range<float>(0.5f, 2.0f);
        auto d = track::HipPrefilter::apply(ctx, st, det, N, MAX_BLOBS, &sub, /*keep_presumed*/ true);
        auto h = track::HipPrefilter::host_policy(st, det, sub, bg.data(), W, 1.0);
        REQUIRE(h.presumed_nr == d.presumed_nr && h.frames.size() == d.frames.size());
        for (size_t f = 0; f < d.frames.size(); ++f) {
            auto same = [](const std::vector<track::HipPrefilter::Entry>& x, const std::vector<track::HipPrefilter::Entry>& y) {
                if (x.size() != y.size()) return false;
                for (size_t k = 0; k < x.size(); ++k) if (x[k].thresholded != y[k].thresholded || x[k].index != y[k].index) return false;
                return true;
            };
            REQUIRE(same(h.frames[f].filtered, d.frames[f].filtered) && same(h.frames[f].big, d.frames[f].big));
            REQUIRE(h.frames[f].filtered_out.size() == d.frames[f].filtered_out.size());
            for (const auto& o : h.frames[f].filtered_out) {
                bool found = false;
                for (const auto& q : d.frames[f].filtered_out)
                    found |= q.entry.thresholded == o.entry.thresholded && q.entry.index == o.entry.index && q.reason == o.reason;
                REQUIRE(found);
            }
        }
        // the device copy of presumed_nr handed over for trexhip_split_search_device holds the same values
        REQUIRE(d.d_presumed_nr != nullptr);
        std::vector<int32_t> back(det.total_blobs);
        REQUIRE(trexhip_copy_to_host(ctx, back.data(), d.d_presumed_nr, back.size() * sizeof(int32_t)) == 0);
        REQUIRE(back == d.presumed_nr);
        trexhip_device_free(ctx, d.d_presumed_nr);
    }
    st.track_threshold_2 = 0;
    // more than 8 ranges: refused, as an exception with the library's message
    st.track_size_filter.assign(9, cmn::Range<double>(1, 2));
    bool threw = false;
    try { track::HipPrefilter::apply(ctx, st, det, N, MAX_BLOBS); } catch (const std::runtime_error& e) { threw = std::strstr(e.what(), "8 ranges") != nullptr; }
    REQUIRE(threw);
    trexhip_destroy(ctx);
    std::printf("prefilter adapter ok\n");
    return 0;
}
