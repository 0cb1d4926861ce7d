// HipVisualField.h -- track::VisualField (Application/src/tracker/tracking/VisualField.h, VisualField.cpp) on libtrexhip, for a batch of
// frames and any number of observers in one call:
//   HipVisualField::calculate(ctx, settings, d_outline, d_posture_info, batch) -> one HipVisualField per observer, with the reference's
//       accessor names: eyes()[j]._depth / _visible_ids / _visible_points / _fov / _visible_head_distance, field_resolution, layers,
//       symmetric_fov, invalid_value.  It builds the entries and observers of trexhip_visual_field_device, makes ONE call and ONE copy
//       back (all outputs live in one device allocation).
//   HipVisualField::cast_host(settings, outline, posture_info, batch) -> the same objects on one host thread: the HOST TWIN of the rule,
//       the reference's functions line by line (tesselate_outline :339-359, project_angles_1d :74-94, plot_projected_line :96-150,
//       add_line and the loop over the active individuals :427-496, :526-576).  It restates tests/visual_field_ref.py in C++ and is
//       what tools/time_visual_field.py times the device call against.
// What stays with the caller (include/trexhip.h says why): VisualField::generate_eyes (a public static of the reference: hand over its
// eyes), and the look-back over max_back_view frames (name the posture row of whichever frame's outline was found).
// Refused loudly (std::invalid_argument): non-empty visual_field_shapes (commons' poly_convex_hull) and gui_pose_smoothing > 0.
// Bit equality with the device and the Python restatement needs every float / double operation rounded on its own: build the including
// unit with -ffp-contract=off where the target has fused multiply-add.  Define TREXHIP_VF_HOST_ONLY to leave out calculate() and with
// it every reference to the library (the host twin then needs nothing but this header).
#pragma once
#ifdef TREXHIP_WITH_TREX
#include <commons.pc.h>
#else
#include "trex_types.h"
#endif
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>
#include "../../include/trexhip.h"

namespace track {

class HipVisualField {
public:
    using Scalar64 = double;
    struct Vec64 { Scalar64 x = 0, y = 0; };
    static constexpr uint8_t layers = TREXHIP_VF_LAYERS;
    static constexpr uint16_t field_resolution = TREXHIP_VF_RESOLUTION;
    static constexpr Scalar64 symmetric_fov = 130.0 * (3.14159265358979323846 / 180.0);    // RADIANS(130)
    static constexpr Scalar64 invalid_value = FLT_MAX;

    struct eye {                                       // VisualField.h:24-44
        Scalar64 angle = 0;
        Vec64 pos, rpos;
        std::array<uint8_t, field_resolution * layers> _fov;
        std::array<Scalar64, field_resolution * layers> _depth;
        std::array<cmn::Vec2, field_resolution * layers> _visible_points;
        std::array<int32_t, field_resolution * layers> _visible_ids;        // long_t
        std::array<Scalar64, field_resolution * layers> _visible_head_distance;
        eye() {
            _fov.fill(0u); _depth.fill(invalid_value); _visible_points.fill(cmn::Vec2(0, 0)); _visible_ids.fill(-1); _visible_head_distance.fill(-1.f);
        }
    };

    struct Settings {
        std::vector<std::vector<cmn::Vec2>> visual_field_shapes;     // must be empty
        int32_t gui_pose_smoothing = 0;                               // must be 0
        Scalar64 max_d = 0;                                           // SQR(Tracker::average().cols) + SQR(Tracker::average().rows)
        Scalar64 max_distance = 5;                                    // tesselate_outline's default argument
        int32_t max_points = 512, max_tess_points = 1024;
    };
    struct Individual {                                // one of Tracker::active_individuals(frame), in its order
        int32_t id = -1;                               // Identity::ID()
        int32_t posture_row = -1;                      // row of the posture call's outline / info (of `virtual_frame`); -1 = none
        cmn::Vec2 pos;                                 // bounds().pos() of that blob
        bool inverted = false;                         // _inverted_because_previous: head_index is the tail
    };
    struct Observer {
        int32_t frame = 0, index = 0;                  // frame of the batch, position in that frame's list
        std::array<Vec64, 2> eye_pos;                  // generate_eyes: eye::pos
        std::array<Scalar64, 2> eye_angle{};           //                eye::angle, corrected to (-pi, pi]
    };
    struct Batch {
        std::vector<std::vector<Individual>> frames;
        std::vector<Observer> observers;
    };

    const std::array<eye, 2>& eyes() const { return _eyes; }
    int32_t status() const { return _status; }         // 0 ok, 1 the observer has no usable posture, 2 an outline of its frame exceeded max_tess_points
    int32_t fish_id() const { return _fish_id; }

    // ---- the host twin -------------------------------------------------------------------------------------------------------------
    template <typename T>
    static void correct_angle(T& angle) {               // :67-72
        static const T two_pi = T(2.0 * 3.14159265358979323846);
        while (angle > 3.14159265358979323846) angle -= two_pi;
        while (angle <= -3.14159265358979323846) angle += two_pi;
    }
    static void project_angles_1d(std::tuple<Scalar64, Scalar64>& t, const Scalar64& ref_angle, Scalar64 angle0, Scalar64 angle1) {   // :74-94
        constexpr Scalar64 fov_start = -symmetric_fov, fov_end = symmetric_fov, fov_len = fov_end - fov_start;
        correct_angle(angle0);
        correct_angle(angle1);
        angle0 = angle0 - ref_angle;
        angle1 = angle1 - ref_angle;
        correct_angle(angle0);
        correct_angle(angle1);
        if (angle1 < angle0) std::swap(angle0, angle1);
        std::get<0>(t) = (angle0 >= fov_start && angle0 <= fov_end) ? (angle0 - fov_start) / fov_len * Scalar64(field_resolution) : -1;
        std::get<1>(t) = (angle1 >= fov_start && angle1 <= fov_end) ? (angle1 - fov_start) / fov_len * Scalar64(field_resolution) : -1;
    }
    // :339-359; Vec2 arithmetic in float32, every operation rounded on its own (UNPINNED, include/trexhip.h).  Returns false as soon as
    // the list holds more than `limit` points (the device's capacity)
    static bool tesselate_outline(const float* outline, size_t n, Scalar64 max_distance, size_t limit, std::vector<Vec64>& copy) {
        copy.clear();
        if (n == 0) return true;
        float px = outline[2 * (n - 1)], py = outline[2 * (n - 1) + 1];
        const float md = (float)max_distance;
        for (size_t k = 0; k < n; ++k) {
            const float x = outline[2 * k], y = outline[2 * k + 1];
            float dx = x - px, dy = y - py;
            const float xx = dx * dx, yy = dy * dy;
            const float L = std::sqrt(xx + yy);
            if ((Scalar64)L > max_distance) {
                dx /= L; dy /= L;
                const Scalar64 N = (Scalar64)L / max_distance + 0.5;
                for (int i = 1; i < N - 1; ++i) {
                    const float fi = (float)i;
                    const float tx = dx * fi, ty = dy * fi;
                    const float sx = tx * md, sy = ty * md;
                    copy.push_back(Vec64{(Scalar64)(px + sx), (Scalar64)(py + sy)});
                    if (copy.size() > limit) return false;
                }
            }
            copy.push_back(Vec64{(Scalar64)x, (Scalar64)y});
            if (copy.size() > limit) return false;
            px = x; py = y;
        }
        return true;
    }
    void plot_projected_line(eye& e, std::tuple<Scalar64, Scalar64>& tuple, Scalar64 d, const Vec64& point, int32_t id, Scalar64 hd) const {   // :96-150
        auto x0 = std::get<0>(tuple), x1 = std::get<1>(tuple);
        if (x0 == x1 && x0 == -1) return;
        x0 = (x0 == Scalar64(-1)) ? x1 : std::max(Scalar64(0.0), x0 - Scalar64(1));
        x1 = (x1 == Scalar64(-1)) ? x0 : std::min(static_cast<Scalar64>(field_resolution) - Scalar64(1.0), x1 + Scalar64(1));
        const unsigned start = static_cast<unsigned>(std::max(Scalar64(0.0), x0));
        const unsigned end = static_cast<unsigned>(std::min(static_cast<Scalar64>(field_resolution), std::ceil(x1)));
        auto fov_of = [this](Scalar64 dd) {
            const Scalar64 v = 1.0 - std::min(1.0, std::max(0.0, dd / _max_d));
            return (uint8_t)(v * v * 255);
        };
        for (unsigned i = start; i <= end && i < field_resolution; ++i) {
            if (e._depth[i] > d) {
                if (e._visible_ids[i] != _fish_id && e._visible_ids[i] != id && e._depth[i + field_resolution] > e._depth[i]) {
                    e._depth[i + field_resolution] = e._depth[i];
                    e._visible_ids[i + field_resolution] = e._visible_ids[i];
                    e._visible_points[i + field_resolution] = e._visible_points[i];
                    e._fov[i + field_resolution] = e._fov[i];
                    e._visible_head_distance[i + field_resolution] = e._visible_head_distance[i];
                }
                e._depth[i] = d;
                e._visible_ids[i] = id;
                e._visible_points[i] = cmn::Vec2((float)point.x, (float)point.y);
                e._fov[i] = fov_of(d);
                e._visible_head_distance[i] = hd;
                if (id == _fish_id) {                                            /* remove 2. stage after self occlusions */
                    if (e._depth[i + field_resolution] != invalid_value) e._depth[i + field_resolution] = invalid_value;
                }
            } else if (e._visible_ids[i] != _fish_id && id != e._visible_ids[i] && e._depth[i + field_resolution] > d) {
                e._depth[i + field_resolution] = d;
                e._visible_ids[i + field_resolution] = id;
                e._visible_points[i + field_resolution] = cmn::Vec2((float)point.x, (float)point.y);
                e._fov[i + field_resolution] = fov_of(d);
                e._visible_head_distance[i + field_resolution] = hd;
            }
        }
    }
    // the add_line lambda (:427-496): left / right from the TARGET's tail index, hd from the OBSERVER's (the lambda captured the outer midline)
    void add_line(int32_t id, const Vec64& pos, const std::vector<Vec64>& points, Scalar64 left_side, Scalar64 right_side, long observer_tail) {
        if (points.empty()) return;
        if (left_side == 0) left_side = points.size() - right_side;
        if (right_side == 0) right_side = points.size() - left_side;
        for (auto& e : _eyes) e.rpos = Vec64{pos.x - e.pos.x, pos.y - e.pos.y};
        auto previous = points[points.size() - 1];
        auto _ptp = points[(points.size() - 2) % points.size()];
        Vec64 line0, line1, rp;
        Scalar64 hd;
        std::tuple<Scalar64, Scalar64> p0;
        for (size_t i = 0; i < points.size(); i++) {
            const Vec64 _pt0 = previous;
            const Vec64 _pt1 = points[i];
            for (const auto& [pt0, pt1] : std::array<std::pair<Vec64, Vec64>, 2>{std::pair<Vec64, Vec64>{_pt0, _pt1}, std::pair<Vec64, Vec64>{_ptp, _pt1}}) {
                hd = 1 - std::abs(Scalar64(i) - Scalar64(observer_tail)) / (((long)i > observer_tail ? left_side : right_side) + 1);
                hd *= 255;
                for (auto& e : _eyes) {
                    line0 = Vec64{pt0.x + e.rpos.x, pt0.y + e.rpos.y};
                    line1 = Vec64{pt1.x + e.rpos.x, pt1.y + e.rpos.y};
                    project_angles_1d(p0, e.angle, std::atan2(line0.y, line0.x), std::atan2(line1.y, line1.x));
                    if (std::get<0>(p0) >= 0 || std::get<1>(p0) >= 0) {
                        if (std::get<0>(p0) >= 0) rp = Vec64{pt0.x + pos.x, pt0.y + pos.y};
                        else rp = Vec64{pt1.x + pos.x, pt1.y + pos.y};
                        const Scalar64 ax = rp.x - e.pos.x, ay = rp.y - e.pos.y;
                        const Scalar64 sx = ax * ax, sy = ay * ay;
                        const Scalar64 d = sx + sy;
                        plot_projected_line(e, p0, d, rp, id, hd);
                    }
                }
            }
            _ptp = previous;
            previous = _pt1;
        }
    }

    static void refuse_unsupported(const Settings& st) {
        if (!st.visual_field_shapes.empty())
            throw std::invalid_argument("HipVisualField: visual_field_shapes is not implemented (poly_convex_hull is not in the tree); it must be empty");
        if (st.gui_pose_smoothing > 0) throw std::invalid_argument("HipVisualField: gui_pose_smoothing > 0 is not implemented");
    }

    // outline: host float2 [rows][max_points]; posture_info: host [rows] -- what the posture call wrote, copied back
    static std::vector<HipVisualField> cast_host(const Settings& st, const float* outline, const trexhip_posture_info* posture_info, const Batch& batch) {
        refuse_unsupported(st);
        auto tail_of = [&](const Individual& a) -> long {
            const trexhip_posture_info& pi = posture_info[a.posture_row];
            return a.inverted ? pi.head_index : pi.tail_index;
        };
        auto used = [&](const Individual& a) { return a.posture_row >= 0 && posture_info[a.posture_row].n_outline > 0 && tail_of(a) != -1; };   // :552
        std::vector<HipVisualField> out(batch.observers.size());
        // tessellated once per used individual of a frame, shared by the frame's observers
        std::vector<std::vector<std::vector<Vec64>>> tess(batch.frames.size());
        std::vector<char> done(batch.frames.size(), 0), over(batch.frames.size(), 0);
        for (size_t o = 0; o < batch.observers.size(); ++o) {
            const Observer& ob = batch.observers[o];
            if (ob.frame < 0 || (size_t)ob.frame >= batch.frames.size() || ob.index < 0 || (size_t)ob.index >= batch.frames[ob.frame].size())
                throw std::invalid_argument("HipVisualField: an observer lies outside its frame");
            const auto& active = batch.frames[ob.frame];
            if (!done[ob.frame]) {
                done[ob.frame] = 1;
                tess[ob.frame].resize(active.size());
                for (size_t k = 0; k < active.size(); ++k)
                    if (used(active[k]) &&
                        !tesselate_outline(outline + (size_t)active[k].posture_row * st.max_points * 2, (size_t)posture_info[active[k].posture_row].n_outline,
                                           st.max_distance, (size_t)st.max_tess_points, tess[ob.frame][k]))
                        over[ob.frame] = 1;
            }
            HipVisualField& vf = out[o];
            vf._max_d = st.max_d;
            vf._fish_id = active[ob.index].id;
            if (over[ob.frame]) { vf._status = 2; continue; }
            if (!used(active[ob.index])) { vf._status = 1; continue; }
            for (int j = 0; j < 2; ++j) { vf._eyes[j].pos = ob.eye_pos[j]; vf._eyes[j].angle = ob.eye_angle[j]; }
            const long observer_tail = tail_of(active[ob.index]);
            for (size_t k = 0; k < active.size(); ++k) {
                const Individual& a = active[k];
                if (!used(a)) continue;
                const auto& points = tess[ob.frame][k];
                const long T = tail_of(a);
                Scalar64 right_side = T + 1;
                Scalar64 left_side = points.size() - T;                           // size_t arithmetic, as written (:572)
                vf.add_line(a.id, Vec64{(Scalar64)a.pos.x, (Scalar64)a.pos.y}, points, left_side, right_side, observer_tail);
            }
        }
        return out;
    }

#ifndef TREXHIP_VF_HOST_ONLY
    // d_outline / d_posture_info: device memory, what trexhip_posture_device / trexhip_posture_auto_device wrote with st.max_points
    static std::vector<HipVisualField> calculate(trexhip_ctx* ctx, const Settings& st, const float* d_outline, const trexhip_posture_info* d_posture_info,
                                                 const Batch& batch) {
        refuse_unsupported(st);
        auto check = [](int rc) { if (rc != 0) throw std::runtime_error(std::string("libtrexhip: ") + trexhip_last_error()); };
        std::vector<int32_t> offsets(1, 0);
        std::vector<trexhip_vf_entry> entries;
        for (const auto& frame : batch.frames) {
            for (const auto& a : frame) entries.push_back(trexhip_vf_entry{a.id, a.posture_row, a.pos.x, a.pos.y, a.inverted ? 1 : 0, 0});
            offsets.push_back((int32_t)entries.size());
        }
        std::vector<trexhip_vf_observer> observers;
        for (const auto& ob : batch.observers) {
            if (ob.frame < 0 || (size_t)ob.frame >= batch.frames.size()) throw std::invalid_argument("HipVisualField: an observer lies outside its frame");
            trexhip_vf_observer v;
            v.frame = ob.frame; v.entry = offsets[ob.frame] + ob.index;
            for (int j = 0; j < 2; ++j) { v.eye_x[j] = ob.eye_pos[j].x; v.eye_y[j] = ob.eye_pos[j].y; v.eye_angle[j] = ob.eye_angle[j]; }
            observers.push_back(v);
        }
        const size_t no = observers.size(), cells = no * 2 * layers * field_resolution;
        std::vector<HipVisualField> out(no);
        if (no == 0) return out;
        trexhip_vf_params vp;
        trexhip_default_vf_params(ctx, &vp);
        vp.max_d = st.max_d; vp.max_distance = st.max_distance; vp.max_points = st.max_points; vp.max_tess_points = st.max_tess_points;
        std::vector<void*> owned;
        struct Free { trexhip_ctx* c; std::vector<void*>& v; ~Free() { for (void* p : v) if (p) trexhip_device_free(c, p); } } guard{ctx, owned};
        auto alloc = [&](size_t bytes) { void* p = nullptr; check(trexhip_device_alloc(ctx, bytes ? bytes : 16, &p)); owned.push_back(p); return p; };
        auto upload = [&](const void* src, size_t bytes) { void* p = alloc(bytes); if (bytes) check(trexhip_copy_to_device(ctx, p, src, bytes)); return p; };
        const auto* d_off = static_cast<const int32_t*>(upload(offsets.data(), offsets.size() * sizeof(int32_t)));
        const auto* d_ent = static_cast<const trexhip_vf_entry*>(upload(entries.data(), entries.size() * sizeof(trexhip_vf_entry)));
        const auto* d_obs = static_cast<const trexhip_vf_observer*>(upload(observers.data(), observers.size() * sizeof(trexhip_vf_observer)));
        // one allocation for every output, widest first so that each part is aligned: depth | head distance | points | ids | status | fov
        const size_t o_depth = 0, o_hd = o_depth + cells * 8, o_pts = o_hd + cells * 8, o_ids = o_pts + cells * 8, o_status = o_ids + cells * 4,
                     o_fov = o_status + no * 4, total = o_fov + cells;
        uint8_t* d_all = static_cast<uint8_t*>(alloc(total));
        check(trexhip_visual_field_device(ctx, &vp, d_outline, d_posture_info, d_off, (int32_t)batch.frames.size(), d_ent, (int32_t)entries.size(), d_obs,
                                          (int32_t)no, reinterpret_cast<double*>(d_all + o_depth), reinterpret_cast<int32_t*>(d_all + o_ids),
                                          reinterpret_cast<float*>(d_all + o_pts), d_all + o_fov, reinterpret_cast<double*>(d_all + o_hd),
                                          reinterpret_cast<int32_t*>(d_all + o_status)));
        std::vector<uint8_t> host(total);
        check(trexhip_copy_to_host(ctx, host.data(), d_all, total));
        const size_t per = (size_t)layers * field_resolution;
        for (size_t o = 0; o < no; ++o) {
            HipVisualField& vf = out[o];
            vf._max_d = st.max_d;
            vf._fish_id = entries[observers[o].entry].id;
            std::memcpy(&vf._status, host.data() + o_status + o * 4, 4);
            for (size_t j = 0; j < 2; ++j) {
                eye& e = vf._eyes[j];
                e.pos = batch.observers[o].eye_pos[j]; e.angle = batch.observers[o].eye_angle[j];
                const size_t at = (o * 2 + j) * per;
                std::memcpy(e._depth.data(), host.data() + o_depth + at * 8, per * 8);
                std::memcpy(e._visible_head_distance.data(), host.data() + o_hd + at * 8, per * 8);
                std::memcpy(static_cast<void*>(e._visible_points.data()), host.data() + o_pts + at * 8, per * 8);
                std::memcpy(e._visible_ids.data(), host.data() + o_ids + at * 4, per * 4);
                std::memcpy(e._fov.data(), host.data() + o_fov + at, per);
            }
        }
        return out;
    }
#endif

private:
    std::array<eye, 2> _eyes;
    Scalar64 _max_d = 0;
    int32_t _fish_id = -1, _status = 0;
};

}  // namespace track
