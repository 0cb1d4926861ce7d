// The host side of tools/time_visual_field.py: track::HipVisualField::cast_host, the host twin of the device rule, on one thread, on the
// scene the tool wrote (the layout of tests/cpp/test_visual_field.cpp's vectors; its expected outputs are what the device call gave).
// Prints one line: microseconds per call for every repetition, then the number of cells that differ from the device's depth / ids.
// No library, no device: built with -DTREXHIP_VF_HOST_ONLY.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>
#include "../trex_amd/host/HipVisualField.h"

using VF = track::HipVisualField;

template <typename T>
static bool read_vec(std::ifstream& f, std::vector<T>& v, size_t n) {
    v.resize(n);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    return (bool)f;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int reps = std::atoi(argv[2]);
    std::ifstream f(argv[1], std::ios::binary);
    int32_t h[7];
    double d[2];
    f.read(reinterpret_cast<char*>(h), sizeof h);                      // count (1), rows, max_points, n_frames, n_entries, n_observers, max_tess
    f.read(reinterpret_cast<char*>(d), sizeof d);
    if (!f || h[0] != 1) return 2;
    std::vector<float> outline;
    std::vector<trexhip_posture_info> info;
    std::vector<int32_t> offsets, ids;
    std::vector<trexhip_vf_entry> entries;
    std::vector<trexhip_vf_observer> observers;
    std::vector<double> depth;
    const size_t cells = (size_t)h[5] * 2 * 2 * 512;
    if (!(read_vec(f, outline, (size_t)h[1] * h[2] * 2) && read_vec(f, info, (size_t)h[1]) && read_vec(f, offsets, (size_t)h[3] + 1) &&
          read_vec(f, entries, (size_t)h[4]) && read_vec(f, observers, (size_t)h[5]) && read_vec(f, depth, cells) && read_vec(f, ids, cells)))
        return 2;
    VF::Settings st;
    st.max_d = d[0]; st.max_distance = d[1]; st.max_points = h[2]; st.max_tess_points = h[6];
    VF::Batch b;
    b.frames.resize(h[3]);
    for (int fr = 0; fr < h[3]; ++fr)
        for (int k = offsets[fr]; k < offsets[fr + 1]; ++k) {
            VF::Individual a;
            a.id = entries[k].id; a.posture_row = entries[k].posture_row; a.pos = cmn::Vec2(entries[k].pos_x, entries[k].pos_y); a.inverted = entries[k].flags & 1;
            b.frames[fr].push_back(a);
        }
    for (const auto& o : observers) {
        VF::Observer ob;
        ob.frame = o.frame; ob.index = o.entry - offsets[o.frame];
        for (int j = 0; j < 2; ++j) { ob.eye_pos[j] = VF::Vec64{o.eye_x[j], o.eye_y[j]}; ob.eye_angle[j] = o.eye_angle[j]; }
        b.observers.push_back(ob);
    }
    size_t differ = 0;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        const auto out = VF::cast_host(st, outline.data(), info.data(), b);
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("%.1f ", std::chrono::duration<double, std::micro>(t1 - t0).count());
        if (r == 0)
            for (size_t o = 0; o < out.size(); ++o)
                for (size_t j = 0; j < 2; ++j)
                    for (size_t i = 0; i < 1024; ++i)
                        differ += std::memcmp(&out[o].eyes()[j]._depth[i], &depth[(o * 2 + j) * 1024 + i], 8) != 0 || out[o].eyes()[j]._visible_ids[i] != ids[(o * 2 + j) * 1024 + i];
    }
    std::printf("differ %zu\n", differ);
    return 0;
}
