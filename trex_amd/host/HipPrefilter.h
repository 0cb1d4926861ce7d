// HipPrefilter.h -- Tracker::prefilter's blob policy (Application/src/tracker/tracking/Tracker.cpp:742-914) on libtrexhip:
//   HipPrefilter::apply(ctx, settings, det, max_batch, max_blobs, &sub) -> per frame `filtered`, `filtered_out` with its reason and the big
//   list; det = the batch trexhip_fetch returned.  One trexhip_prefilter_device call on the context's last fetched batch (segmented or
//   loaded) and one copy of its four small outputs.  presumed_nr comes back as a host copy (Result::presumed_nr, pooled order of the detect
//   table); with Result::d_presumed_nr requested (keep_presumed = true) the device array the call wrote is handed over as well, owned by
//   the caller (trexhip_device_free), in the form trexhip_split_search_device takes, so the split search starts without an upload.
//   HipPrefilter::host_policy(settings, det, sub, background, ...) -> the same Result from the two fetched table sets on one host thread:
//   the route a caller had to take before trexhip_prefilter_device (re-threshold, fetch, this loop, upload of presumed_nr).  It restates
//   tests/prefilter_ref.py in C++ and is what tools/time_prefilter.py times the device call against.
// An entry names a blob by table and pooled index: `thresholded` = a sub-blob of the second table set (trexhip_fetch_rethreshold),
// else the detect blob itself (trexhip_fetch).  Packing of the shape and bdx tables is plain host code (pack_shapes / pack_bdx).
#pragma once
#ifdef TREXHIP_WITH_TREX
#include <commons.pc.h>
#else
#include "trex_types.h"
#endif
#include <cstdint>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/trexhip.h"

namespace track {

struct HipPrefilter {
    struct Settings {
        int32_t track_threshold = 15, method = 0, track_threshold_2 = 0;
        cmn::Range<float> threshold_ratio_range{0.5f, 1.0f};
        std::vector<cmn::Range<double>> track_size_filter;
        std::vector<std::vector<cmn::Vec2>> track_include, track_ignore;
        std::vector<std::set<uint32_t>> track_ignore_bdx;        // per frame of the batch (empty vector = the setting is empty)
    };
    struct Entry { bool thresholded = false; uint32_t index = 0; };   // pooled index: sub.blobs[index] when thresholded, else det.blobs[index]
    struct FilteredOut { Entry entry; int32_t reason = 0; };     // TREXHIP_FILTER_*
    struct Frame {
        std::vector<Entry> filtered, big;
        std::vector<FilteredOut> filtered_out;
        bool undecided = false;                                   // the frame overflowed or was malformed
    };
    struct Result {
        std::vector<Frame> frames;
        std::vector<int32_t> presumed_nr;                         // per detect blob, pooled order
        int32_t* d_presumed_nr = nullptr;                         // apply(..., keep_presumed = true): the same on the device, the caller frees it
    };
    struct Tables {
        std::vector<float> points;
        std::vector<int32_t> offsets;
    };

    static Tables pack_shapes(const std::vector<std::vector<cmn::Vec2>>& shapes) {
        Tables t;
        t.offsets.push_back(0);
        for (const auto& s : shapes) {
            for (const auto& p : s) { t.points.push_back(p.x); t.points.push_back(p.y); }
            t.offsets.push_back((int32_t)(t.points.size() / 2));
        }
        return t;
    }
    static void pack_bdx(const std::vector<std::set<uint32_t>>& per_frame, int32_t n_frames, std::vector<uint32_t>& words, std::vector<int32_t>& offsets) {
        words.clear();
        offsets.assign(1, 0);
        for (int32_t f = 0; f < n_frames; ++f) {
            if ((size_t)f < per_frame.size()) words.insert(words.end(), per_frame[f].begin(), per_frame[f].end());   // std::set iterates sorted
            offsets.push_back((int32_t)words.size());
        }
    }

    // det = the batch trexhip_fetch returned (segmented or loaded); max_batch / max_blobs = the context's capacities.  *sub_out receives the
    // second table set (trexhip_fetch_rethreshold: the sub-blobs the thresholded entries name; its frame ranges sort filtered_out by frame)
    static Result apply(trexhip_ctx* ctx, const Settings& st, const trexhip_batch_result& det, int32_t max_batch, int32_t max_blobs,
                        trexhip_batch_result* sub_out = nullptr, bool keep_presumed = false) {
        auto check = [](int rc) { if (rc != 0) throw std::runtime_error(std::string("libtrexhip: ") + trexhip_last_error()); };
        const int32_t n_frames = det.n_frames;
        const uint32_t total_blobs = det.total_blobs;
        trexhip_prefilter_params pp;
        trexhip_default_prefilter_params(&pp);
        pp.track_threshold = st.track_threshold; pp.method = st.method; pp.track_threshold_2 = st.track_threshold_2;
        pp.threshold_ratio_range[0] = st.threshold_ratio_range.start; pp.threshold_ratio_range[1] = st.threshold_ratio_range.end;
        pp.n_ranges = (int32_t)st.track_size_filter.size();
        for (size_t i = 0; i < st.track_size_filter.size() && i < 8; ++i) {
            pp.size_ranges[2 * i] = st.track_size_filter[i].start; pp.size_ranges[2 * i + 1] = st.track_size_filter[i].end;
        }
        const size_t cap = (size_t)max_batch * (size_t)max_blobs, per_frame = 2 * (size_t)max_blobs;
        std::vector<void*> owned;
        struct Free { trexhip_ctx* c; std::vector<void*>& v; ~Free() { for (void* p : v) if (p) trexhip_device_free(c, p); } } guard{ctx, owned};
        auto alloc = [&](size_t bytes) { void* p = nullptr; check(trexhip_device_alloc(ctx, bytes ? bytes : 4, &p)); owned.push_back(p); return p; };
        auto upload = [&](const void* src, size_t bytes) { void* p = alloc(bytes); if (bytes) check(trexhip_copy_to_device(ctx, p, src, bytes)); return p; };
        trexhip_prefilter_tables tb = {};
        const Tables inc = pack_shapes(st.track_include), ign = pack_shapes(st.track_ignore);
        if (!st.track_include.empty()) {
            tb.d_include_points = static_cast<const float*>(upload(inc.points.data(), inc.points.size() * sizeof(float)));
            tb.d_include_offsets = static_cast<const int32_t*>(upload(inc.offsets.data(), inc.offsets.size() * sizeof(int32_t)));
            tb.n_include_shapes = (int32_t)st.track_include.size(); tb.n_include_points = (int32_t)(inc.points.size() / 2);
        }
        if (!st.track_ignore.empty()) {
            tb.d_ignore_points = static_cast<const float*>(upload(ign.points.data(), ign.points.size() * sizeof(float)));
            tb.d_ignore_offsets = static_cast<const int32_t*>(upload(ign.offsets.data(), ign.offsets.size() * sizeof(int32_t)));
            tb.n_ignore_shapes = (int32_t)st.track_ignore.size(); tb.n_ignore_points = (int32_t)(ign.points.size() / 2);
        }
        if (!st.track_ignore_bdx.empty()) {
            std::vector<uint32_t> words;
            std::vector<int32_t> offsets;
            pack_bdx(st.track_ignore_bdx, n_frames, words, offsets);
            tb.d_ignore_bdx = static_cast<const uint32_t*>(upload(words.data(), words.size() * sizeof(uint32_t)));
            tb.d_ignore_bdx_offsets = static_cast<const int32_t*>(upload(offsets.data(), offsets.size() * sizeof(int32_t)));
            tb.n_ignore_bdx = (int32_t)words.size();
        }
        uint8_t* d_decision = static_cast<uint8_t*>(alloc(2 * cap));
        int32_t* d_order = static_cast<int32_t*>(alloc(sizeof(int32_t) * (size_t)n_frames * per_frame));
        int32_t* d_counts = static_cast<int32_t*>(alloc(sizeof(int32_t) * 4 * (size_t)n_frames));
        int32_t* d_presumed = static_cast<int32_t*>(alloc(sizeof(int32_t) * (size_t)total_blobs));
        check(trexhip_prefilter_device(ctx, &pp, &tb, d_decision, d_order, d_counts, d_presumed));
        std::vector<uint8_t> decision(2 * cap);
        std::vector<int32_t> order((size_t)n_frames * per_frame), counts(4 * (size_t)n_frames);
        Result out;
        out.presumed_nr.resize(total_blobs);
        check(trexhip_copy_to_host(ctx, decision.data(), d_decision, decision.size()));
        check(trexhip_copy_to_host(ctx, order.data(), d_order, order.size() * sizeof(int32_t)));
        check(trexhip_copy_to_host(ctx, counts.data(), d_counts, counts.size() * sizeof(int32_t)));
        if (total_blobs) check(trexhip_copy_to_host(ctx, out.presumed_nr.data(), d_presumed, out.presumed_nr.size() * sizeof(int32_t)));
        trexhip_batch_result sub;
        const int rc = trexhip_fetch_rethreshold(ctx, &sub);
        if (rc != 0 && rc != TREXHIP_E_CAPACITY) check(rc);                        // an overflowed frame is reported per frame (undecided)
        if (sub_out) *sub_out = sub;
        if (keep_presumed) {                                                       // out of the guard's hands: the caller owns it now
            for (auto& p : owned) if (p == d_presumed) p = nullptr;
            out.d_presumed_nr = d_presumed;
        }
        // entry f * max_blobs + k = sub-blob k of frame f, cap + f * max_blobs + k = its detect blob k; Entry::index is the pooled index
        auto entry_of = [&](int32_t f, size_t e) {
            Entry en;
            en.thresholded = e < cap;
            const size_t k = (e < cap ? e : e - cap) - (size_t)f * (size_t)max_blobs;
            en.index = (uint32_t)((en.thresholded ? sub.frames[f].blob_begin : det.frames[f].blob_begin) + k);
            return en;
        };
        out.frames.resize((size_t)n_frames);
        for (int32_t f = 0; f < n_frames; ++f) {
            Frame& fr = out.frames[(size_t)f];
            fr.undecided = counts[4 * (size_t)f + 3] != 0;
            if (fr.undecided) continue;
            const int32_t* ord = order.data() + (size_t)f * per_frame;
            const int32_t nc = counts[4 * (size_t)f], nb = counts[4 * (size_t)f + 1];
            for (int32_t k = 0; k < nc; ++k) fr.filtered.push_back(entry_of(f, (size_t)ord[k]));
            for (int32_t k = 0; k < nb; ++k) fr.big.push_back(entry_of(f, (size_t)ord[nc + k]));
            // filtered_out in table order: the frame's detect blobs (imprecise check, un-thresholded entries), then its sub-blobs
            auto collect = [&](size_t begin, size_t n) {
                for (size_t e = begin; e < begin + n; ++e)
                    if (decision[e] >= TREXHIP_DECISION_FILTERED && decision[e] != TREXHIP_DECISION_NONE)
                        fr.filtered_out.push_back(FilteredOut{entry_of(f, e), (int32_t)decision[e] - TREXHIP_DECISION_FILTERED});
            };
            collect(cap + (size_t)f * (size_t)max_blobs, det.frames[f].n_blobs);
            collect((size_t)f * (size_t)max_blobs, sub.frames[f].n_blobs);
        }
        return out;
    }

    // ---- the same policy on the host, from the two fetched table sets (the C++ twin of tests/prefilter_ref.py) ---------------------------
    // bg: the background image (grey, `bg_stride` bytes per row); cm_per_pixel: the context's live value.  Frames flagged in either table
    // set are undecided.  filtered_out is in the order the reference's loop filters (apply() lists it in table order).
    static Result host_policy(const Settings& st, const trexhip_batch_result& det, const trexhip_batch_result& sub, const uint8_t* bg,
                              size_t bg_stride, double cm_per_pixel) {
        const float cm_sqr = (float)(cm_per_pixel * cm_per_pixel);
        const auto& ranges = st.track_size_filter;
        double mr_start = -1, mr_end = -1;                                         // SizeFilters::max_range (SizeFilters.cpp:12-18)
        for (const auto& r : ranges) {
            if (mr_start == -1 || r.start < mr_start) mr_start = r.start;
            if (mr_end == -1 || r.end > mr_end) mr_end = r.end;
        }
        auto in_range = [&](float v) {                                             // in_range_of_one (:36-53)
            if (ranges.empty()) return true;
            for (const auto& r : ranges) if ((double)v >= r.start && (double)v < r.end) return true;
            return false;
        };
        auto close_to_minimum = [&](float v) {                                     // close_to_minimum_of_one(v, 0.5) (:20-26)
            for (const auto& r : ranges) if ((double)v >= r.start * (double)0.5f) return true;
            return false;
        };
        auto matches = [](const trexhip_blob& B, const std::vector<std::vector<cmn::Vec2>>& shapes) {   // PrefilterBlobs.cpp:328-355
            const float cx = (float)B.x0 + (float)(B.x1 - B.x0 + 1) * 0.5f, cy = (float)B.y0 + (float)(B.y1 - B.y0 + 1) * 0.5f;
            for (const auto& s : shapes) {
                const size_t n = s.size();
                if (n == 2) {
                    const float x = s[0].x, y = s[0].y, w = s[1].x - x, h = s[1].y - y;
                    if (cx >= x && cx < x + w && cy >= y && cy < y + h) return true;
                } else if (n > 2) {
                    bool in = false;
                    for (size_t i = 0, j = n - 1; i < n; j = i++)
                        if (((s[i].y > cy) != (s[j].y > cy)) && (cx < (s[j].x - s[i].x) * (cy - s[i].y) / (s[j].y - s[i].y) + s[i].x)) in = !in;
                    if (in) return true;
                }
            }
            return false;
        };
        auto overlaps = [](const trexhip_blob& B, const std::vector<std::vector<cmn::Vec2>>& shapes) {  // PrefilterBlobs.cpp:357-385
            const float bx = (float)B.x0, by = (float)B.y0, bw = (float)(B.x1 - B.x0 + 1), bh = (float)(B.y1 - B.y0 + 1);
            for (const auto& s : shapes) {
                float x, y, w, h;
                if (s.size() == 2) { x = s[0].x; y = s[0].y; w = s[1].x - x; h = s[1].y - y; }
                else if (s.size() > 2) {
                    x = 0.f; y = 0.f; w = 3.402823466e+38f; h = 3.402823466e+38f;
                    for (const auto& p : s) { x = p.x < x ? p.x : x; y = p.y < y ? p.y : y; w = p.x > w ? p.x : w; h = p.y > h ? p.y : h; }
                    w -= x; h -= y;
                } else continue;
                if (x < bx + bw && bx < x + w && y < by + bh && by < y + h) return true;
            }
            return false;
        };
        auto diff = [&](int p, int b) { return st.method == 0 ? (b > p ? b - p : p - b) : (st.method == 1 ? (b > p ? b - p : 0) : p); };
        Result out;
        out.frames.resize((size_t)det.n_frames);
        out.presumed_nr.assign(det.total_blobs, 0);
        std::vector<std::vector<uint32_t>> children;
        std::vector<uint32_t> survivors;
        for (int32_t f = 0; f < det.n_frames; ++f) {
            Frame& fr = out.frames[(size_t)f];
            const trexhip_frame_info &f1 = det.frames[f], &f2 = sub.frames[f];
            fr.undecided = f1.flags != 0 || f2.flags != 0;
            if (fr.undecided) continue;
            const std::set<uint32_t>* ignore = (size_t)f < st.track_ignore_bdx.size() ? &st.track_ignore_bdx[(size_t)f] : nullptr;
            children.assign(f1.n_blobs, {});
            survivors.assign(f1.n_blobs, 0u);
            for (uint32_t i = 0; i < f2.n_blobs; ++i) {
                const uint32_t p = sub.blobs[f2.blob_begin + i].parent - f1.blob_begin;
                if (p < f1.n_blobs) { children[p].push_back(f2.blob_begin + i); survivors[p] += sub.blobs[f2.blob_begin + i].n_pixels; }
            }
            auto blob_of = [&](const Entry& e) -> const trexhip_blob& { return e.thresholded ? sub.blobs[e.index] : det.blobs[e.index]; };
            auto filter_out = [&](const Entry& e, int32_t reason) { fr.filtered_out.push_back(FilteredOut{e, reason}); };
            auto bdx_ignored = [&](const Entry& e, uint32_t parent) {               // PrefilterBlobs.cpp:130-150
                if (!ignore) return false;
                return ignore->count(blob_of(e).bid) > 0 || (e.thresholded && ignore->count(det.blobs[parent].bid) > 0);
            };
            auto precise = [&](const Entry& e, uint32_t parent) {                   // check_precise_not_ignored (:742-763)
                const trexhip_blob& B = blob_of(e);
                if (!st.track_ignore.empty() && matches(B, st.track_ignore)) { filter_out(e, TREXHIP_FILTER_INSIDE_IGNORE); return false; }
                if (!st.track_include.empty() && !matches(B, st.track_include)) { filter_out(e, TREXHIP_FILTER_OUTSIDE_INCLUDE); return false; }
                if (bdx_ignored(e, parent)) { filter_out(e, TREXHIP_FILTER_BDX_IGNORED); return false; }
                return true;
            };
            auto recount_of = [&](const Entry& e, uint32_t j) {                     // :768-774
                const float full = (float)blob_of(e).n_pixels * cm_sqr;
                if (!ranges.empty() && (double)full > mr_end * 100.0) return full;
                return e.thresholded ? full : (float)survivors[j] * cm_sqr;
            };
            auto second_pixels = [&](const Entry& e) {                              // recount(track_threshold_2) (:866)
                const trexhip_batch_result& t = e.thresholded ? sub : det;
                const trexhip_frame_info& fi = e.thresholded ? f2 : f1;
                const trexhip_blob& B = blob_of(e);
                const trexhip_run* rr = t.runs + fi.run_begin + B.run_begin;
                const uint8_t* px = t.pixels + fi.pix_begin + B.pix_begin;
                uint32_t n = 0;
                for (uint32_t r = 0; r < B.n_runs; ++r) {
                    const uint8_t* b = bg + (size_t)rr[r].y * bg_stride;
                    for (uint32_t x = rr[r].x0; x <= rr[r].x1; ++x) n += diff((int)*px++, (int)b[x]) >= st.track_threshold_2;
                }
                return n;
            };
            std::vector<Entry> ptrs;
            for (uint32_t j = 0; j < f1.n_blobs; ++j) {                             // :806
                Entry own; own.thresholded = false; own.index = f1.blob_begin + j;
                if (!st.track_include.empty() && !overlaps(det.blobs[own.index], st.track_include)) { filter_out(own, TREXHIP_FILTER_OUTSIDE_INCLUDE); continue; }
                if (bdx_ignored(own, own.index)) { filter_out(own, TREXHIP_FILTER_BDX_IGNORED); continue; }
                ptrs.clear();
                size_t found = 0;
                if ((ranges.empty() || close_to_minimum(recount_of(own, j))) && st.track_threshold > 0) {   // :828-831
                    found = children[j].size();
                    for (uint32_t i : children[j]) {
                        Entry add; add.thresholded = true; add.index = i;
                        if (precise(add, own.index)) ptrs.push_back(add);
                    }
                }
                if (found == 0) {                                                   // :853-858
                    if (!precise(own, own.index)) continue;
                    ptrs.push_back(own);
                }
                for (const Entry& e : ptrs) {                                       // :861-914
                    const float recount = recount_of(e, j);
                    if (in_range(recount)) {
                        if (st.track_threshold_2 > 0) {
                            const float second_count = (float)second_pixels(e) * cm_sqr;
                            const float lo = st.threshold_ratio_range.start * recount, hi = st.threshold_ratio_range.end * recount;
                            if (!(second_count >= lo && second_count < hi)) { filter_out(e, TREXHIP_FILTER_SECOND_THRESHOLD); continue; }
                        }
                        fr.filtered.push_back(e);
                    } else if (!ranges.empty() && (double)recount < mr_start) filter_out(e, TREXHIP_FILTER_OUTSIDE_RANGE);
                    else { fr.big.push_back(e); out.presumed_nr[own.index] = 2; }   // split_expectation(2, false), PrefilterBlobs.cpp:223
                }
            }
        }
        return out;
    }
};

}  // namespace track
