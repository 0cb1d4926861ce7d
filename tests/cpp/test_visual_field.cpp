// Holds track::HipVisualField (trex_amd/host/HipVisualField.h) to vectors the Python restatement wrote (tests/visual_field_ref.py through
// tests/test_visual_field_cpp.py), byte for byte.
//   test_visual_field FILE            cast_host, the host twin, on every scene of the file.  Built with -DTREXHIP_VF_HOST_ONLY this needs no
//                                     library and no device: plain host code with its own main, also built with the sanitizers.
//   test_visual_field FILE --device   (not host-only) calculate() through the C ABI on every scene, compared with cast_host and the file
// File: int32 count; per scene int32 {rows, max_points, n_frames, n_entries, n_observers, max_tess_points}, double {max_d, max_distance},
// outline float [rows][max_points][2], trexhip_posture_info [rows], int32 offsets [n_frames + 1], trexhip_vf_entry [n_entries],
// trexhip_vf_observer [n_observers], then the expected depth, ids, points, fov, head distance ([n_observers][2][2][512]) and status.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "../../trex_amd/host/HipVisualField.h"

#define REQUIRE(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

using VF = track::HipVisualField;

struct Scene {
    int32_t rows, max_points, n_frames, n_entries, n_observers, max_tess;
    double max_d, max_distance;
    std::vector<float> outline;
    std::vector<trexhip_posture_info> info;
    std::vector<int32_t> offsets;
    std::vector<trexhip_vf_entry> entries;
    std::vector<trexhip_vf_observer> observers;
    std::vector<double> depth, hd;
    std::vector<int32_t> ids, status;
    std::vector<float> points;
    std::vector<uint8_t> fov;
};

template <typename T>
static bool read_vec(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    return (bool)f;
}

static bool read_scene(std::ifstream& f, Scene& s) {
    int32_t h[6];
    double d[2];
    f.read(reinterpret_cast<char*>(h), sizeof h);
    f.read(reinterpret_cast<char*>(d), sizeof d);
    if (!f) return false;
    s.rows = h[0]; s.max_points = h[1]; s.n_frames = h[2]; s.n_entries = h[3]; s.n_observers = h[4]; s.max_tess = h[5];
    s.max_d = d[0]; s.max_distance = d[1];
    const size_t cells = (size_t)s.n_observers * 2 * 2 * 512;
    return read_vec(f, s.outline, (size_t)s.rows * s.max_points * 2) && read_vec(f, s.info, (size_t)s.rows) && read_vec(f, s.offsets, (size_t)s.n_frames + 1) &&
           read_vec(f, s.entries, (size_t)s.n_entries) && read_vec(f, s.observers, (size_t)s.n_observers) && read_vec(f, s.depth, cells) &&
           read_vec(f, s.ids, cells) && read_vec(f, s.points, cells * 2) && read_vec(f, s.fov, cells) && read_vec(f, s.hd, cells) &&
           read_vec(f, s.status, (size_t)s.n_observers);
}

static VF::Batch batch_of(const Scene& s) {
    VF::Batch b;
    b.frames.resize(s.n_frames);
    for (int f = 0; f < s.n_frames; ++f)
        for (int k = s.offsets[f]; k < s.offsets[f + 1]; ++k) {
            VF::Individual a;
            a.id = s.entries[k].id; a.posture_row = s.entries[k].posture_row; a.pos = cmn::Vec2(s.entries[k].pos_x, s.entries[k].pos_y);
            a.inverted = (s.entries[k].flags & 1) != 0;
            b.frames[f].push_back(a);
        }
    for (const auto& o : s.observers) {
        VF::Observer ob;
        ob.frame = o.frame; ob.index = o.entry - s.offsets[o.frame];
        for (int j = 0; j < 2; ++j) { ob.eye_pos[j] = VF::Vec64{o.eye_x[j], o.eye_y[j]}; ob.eye_angle[j] = o.eye_angle[j]; }
        b.observers.push_back(ob);
    }
    return b;
}

// every member of every eye against the file, byte for byte
static int compare(const Scene& s, const std::vector<VF>& got, const char* what, int scene) {
    REQUIRE(got.size() == (size_t)s.n_observers);
    const size_t per = (size_t)VF::layers * VF::field_resolution;
    for (size_t o = 0; o < got.size(); ++o) {
        if (got[o].status() != s.status[o]) { std::printf("FAILED scene %d %s: observer %zu status %d, want %d\n", scene, what, o, got[o].status(), s.status[o]); return 1; }
        for (size_t j = 0; j < 2; ++j) {
            const auto& e = got[o].eyes()[j];
            const size_t at = (o * 2 + j) * per;
            const bool ok = std::memcmp(e._depth.data(), s.depth.data() + at, per * 8) == 0 && std::memcmp(e._visible_ids.data(), s.ids.data() + at, per * 4) == 0 &&
                            std::memcmp(static_cast<const void*>(e._visible_points.data()), s.points.data() + at * 2, per * 8) == 0 &&
                            std::memcmp(e._fov.data(), s.fov.data() + at, per) == 0 &&
                            std::memcmp(e._visible_head_distance.data(), s.hd.data() + at, per * 8) == 0;
            if (!ok) {
                for (size_t i = 0; i < per; ++i)
                    if (std::memcmp(&e._depth[i], &s.depth[at + i], 8) != 0 || e._visible_ids[i] != s.ids[at + i] || e._fov[i] != s.fov[at + i]) {
                        std::printf("scene %d %s: observer %zu eye %zu cell %zu: depth %.17g / %.17g id %d / %d fov %d / %d\n", scene, what, o, j, i, e._depth[i],
                                    s.depth[at + i], e._visible_ids[i], s.ids[at + i], e._fov[i], s.fov[at + i]);
                        break;
                    }
                std::printf("FAILED scene %d %s: observer %zu eye %zu differs from the restatement\n", scene, what, o, j);
                return 1;
            }
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(trexhip_vf_entry) == 24 && sizeof(trexhip_vf_observer) == 56 && sizeof(trexhip_vf_params) == 24 && sizeof(cmn::Vec2) == 8, "layouts");
    static_assert(VF::field_resolution == 512 && VF::layers == 2, "constants");
    REQUIRE(argc >= 2);
    const bool device = argc > 2 && std::strcmp(argv[2], "--device") == 0;
    // the refusals are host code
    {
        VF::Settings st;
        st.gui_pose_smoothing = 1;
        bool threw = false;
        try { VF::cast_host(st, nullptr, nullptr, VF::Batch{}); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
        st.gui_pose_smoothing = 0;
        st.visual_field_shapes = {{cmn::Vec2(0, 0), cmn::Vec2(1, 0), cmn::Vec2(0, 1)}};
        threw = false;
        try { VF::cast_host(st, nullptr, nullptr, VF::Batch{}); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
        REQUIRE(VF::invalid_value == (double)FLT_MAX && VF().eyes()[1]._depth[1023] == VF::invalid_value && VF().eyes()[0]._visible_ids[0] == -1 &&
                VF().eyes()[0]._visible_head_distance[5] == -1.0 && VF().eyes()[0]._fov[7] == 0);
    }
    std::ifstream f(argv[1], std::ios::binary);
    REQUIRE((bool)f);
    int32_t count = 0;
    f.read(reinterpret_cast<char*>(&count), 4);
    REQUIRE(f && count > 0);
#ifndef TREXHIP_VF_HOST_ONLY
    trexhip_ctx* ctx = nullptr;
    if (device) {
        trexhip_params p;
        trexhip_default_params(&p, 640, 480);
        p.max_batch = 1;
        REQUIRE(trexhip_create(&p, &ctx) == 0);
    }
#else
    REQUIRE(!device);
#endif
    for (int k = 0; k < count; ++k) {
        Scene s;
        REQUIRE(read_scene(f, s));
        VF::Settings st;
        st.max_d = s.max_d; st.max_distance = s.max_distance; st.max_points = s.max_points; st.max_tess_points = s.max_tess;
        const VF::Batch b = batch_of(s);
        const auto host = VF::cast_host(st, s.outline.data(), s.info.data(), b);
        if (compare(s, host, "cast_host", k)) return 1;
#ifndef TREXHIP_VF_HOST_ONLY
        if (device) {
            void *d_outline = nullptr, *d_info = nullptr;
            REQUIRE(trexhip_device_alloc(ctx, s.outline.size() * 4 + 16, &d_outline) == 0 && trexhip_device_alloc(ctx, s.info.size() * sizeof(trexhip_posture_info) + 16, &d_info) == 0);
            REQUIRE(trexhip_copy_to_device(ctx, d_outline, s.outline.data(), s.outline.size() * 4) == 0);
            REQUIRE(trexhip_copy_to_device(ctx, d_info, s.info.data(), s.info.size() * sizeof(trexhip_posture_info)) == 0);
            const auto dev = VF::calculate(ctx, st, static_cast<const float*>(d_outline), static_cast<const trexhip_posture_info*>(d_info), b);
            trexhip_device_free(ctx, d_outline);
            trexhip_device_free(ctx, d_info);
            if (compare(s, dev, "calculate", k)) return 1;
            // the adapter's own twin against the device, member by member
            REQUIRE(dev.size() == host.size());
            for (size_t o = 0; o < dev.size(); ++o)
                for (size_t j = 0; j < 2; ++j) {
                    REQUIRE(dev[o].eyes()[j]._depth == host[o].eyes()[j]._depth && dev[o].eyes()[j]._visible_ids == host[o].eyes()[j]._visible_ids);
                    REQUIRE(dev[o].eyes()[j]._fov == host[o].eyes()[j]._fov && dev[o].eyes()[j]._visible_head_distance == host[o].eyes()[j]._visible_head_distance);
                    REQUIRE(dev[o].eyes()[j]._visible_points == host[o].eyes()[j]._visible_points && dev[o].fish_id() == host[o].fish_id());
                }
        }
#endif
    }
#ifndef TREXHIP_VF_HOST_ONLY
    if (ctx) trexhip_destroy(ctx);
#endif
    std::printf(device ? "visual field adapter ok: %d scenes\n" : "visual field host twin ok: %d scenes\n", count);
    return 0;
}
