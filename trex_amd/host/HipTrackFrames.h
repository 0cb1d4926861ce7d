// HipTrackFrames.h -- the track-side way into the library: frames read back from a .pv file become the context's "last batch".
//   pv::Frame frame; frame.read_from(file, idx);  ...  Tracker::prefilter / posture / FilterCache / SplitBlob on its blobs
//       Application/src/ProcessedVideo/pv.cpp:296-420 (read_from), tracking/Tracker.cpp:765-849 (prefilter)
// load() hands a batch of such frames to trexhip_load_frames_v6_device: each frame's masks and pixel arrays are written as a V_6 frame
// body on the host (pv::Frame::serialize, pv.cpp:666-703, in the layout of version V_6), uploaded, loaded and fetched -- after which
// HipSplitBlob, HipPosture, the crop calls and the identity network run on the batch exactly as behind HipBackgroundSubtraction.
// load_bodies() takes the bodies and offsets of trexhip_pv_read_frames directly (a stored data section, no pv::Frame in between).
// Inside a TRex build define TREXHIP_WITH_TREX to get the real pv::Frame / HorizontalLine types.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/trexhip.h"
#ifdef TREXHIP_WITH_TREX
#include <pv.h>
#else
#include "trex_types.h"
#endif

namespace track {

// One frame as a V_6 body appended to `out`: u8 flag 0, u64 timestamp, u16 n, n x {u16 start_y, u16 mask_size, mask_size x {u16 x0,
// u16 x1 << 1 | eol}, pixels}; eol marks the last line of an image row (pv.h:20-23).  Gray frames only: one byte per pixel.
inline void write_frame_body_v6(const pv::Frame& frame, uint64_t timestamp, std::vector<uint8_t>& out) {
    if (frame.encoding() != cmn::meta_encoding_t::gray) throw std::invalid_argument("write_frame_body_v6: the V_6 layout holds gray pixel arrays");
    if (frame.pixels().size() != frame.mask().size()) throw std::invalid_argument("write_frame_body_v6: every object needs its pixel array");
    auto put16 = [&out](uint32_t v) { out.push_back((uint8_t)(v & 0xffu)); out.push_back((uint8_t)(v >> 8)); };
    out.push_back(0);
    for (int k = 0; k < 8; ++k) out.push_back((uint8_t)(timestamp >> (8 * k)));
    put16(frame.n());
    for (size_t b = 0; b < frame.mask().size(); ++b) {
        const std::vector<cmn::HorizontalLine>& lines = *frame.mask()[b];
        const cmn::PixelArray_t& px = *frame.pixels()[b];
        size_t want = 0;
        for (const cmn::HorizontalLine& l : lines) {
            if (l.x1 < l.x0 || l.x1 >= 32768) throw std::invalid_argument("write_frame_body_v6: a line needs x0 <= x1 < 32768 (pv.h:36)");
            want += (size_t)(l.x1 - l.x0 + 1);
        }
        if (px.size() != want) throw std::invalid_argument("write_frame_body_v6: the pixel array does not match the lines");
        put16(lines.empty() ? 0u : lines[0].y);
        put16((uint32_t)lines.size());
        for (size_t j = 0; j < lines.size(); ++j) {
            const uint32_t eol = (j + 1 == lines.size() || lines[j + 1].y != lines[j].y) ? 1u : 0u;
            put16(lines[j].x0);
            put16(((uint32_t)lines[j].x1 << 1) | eol);
        }
        out.insert(out.end(), px.begin(), px.end());
    }
}

class HipTrackFrames {
public:
    explicit HipTrackFrames(trexhip_ctx* ctx) : _ctx(ctx) {}          // must be destroyed before trexhip_destroy(ctx)
    ~HipTrackFrames() { release(); }
    HipTrackFrames(const HipTrackFrames&) = delete;
    HipTrackFrames& operator=(const HipTrackFrames&) = delete;

    // frames (at most max_batch) -> the context's last batch; timestamps: one per frame or empty (zeros).  Returns the fetched tables
    // (owned by the context, valid until its next fetch).
    trexhip_batch_result load(const std::vector<pv::Frame>& frames, const std::vector<uint64_t>& timestamps = {}) {
        if (!timestamps.empty() && timestamps.size() != frames.size()) throw std::invalid_argument("HipTrackFrames::load: one timestamp per frame");
        std::vector<uint8_t> bodies;
        std::vector<uint64_t> offsets;
        for (size_t f = 0; f < frames.size(); ++f) {
            offsets.push_back(bodies.size());
            write_frame_body_v6(frames[f], timestamps.empty() ? 0ull : timestamps[f], bodies);
        }
        offsets.push_back(bodies.size());
        return load_bodies(bodies.data(), offsets.data(), (int32_t)frames.size());
    }

    // bodies / offsets [n + 1] as trexhip_pv_read_frames (or trexhip_pack_frames_v6_device, copied to the host) gives them
    trexhip_batch_result load_bodies(const uint8_t* bodies, const uint64_t* offsets, int32_t n) {
        if (n < 1 || !bodies || !offsets) throw std::invalid_argument("HipTrackFrames::load_bodies: no frames");
        const size_t bytes = (size_t)offsets[n], table = (size_t)(n + 1) * sizeof(uint64_t);
        reserve(bytes + 8 + table);
        uint8_t* d_off = _d + ((bytes + 7) & ~(size_t)7);               // the offsets behind the bodies, 8-byte aligned
        check(trexhip_copy_to_device(_ctx, _d, bodies, bytes));
        check(trexhip_copy_to_device(_ctx, d_off, offsets, table));
        check(trexhip_load_frames_v6_device(_ctx, _d, reinterpret_cast<const uint64_t*>(d_off), n, nullptr));
        trexhip_batch_result res{};
        check(trexhip_fetch(_ctx, &res));                               // a malformed frame (TREXHIP_E_INVALID) or one beyond capacity throws here
        return res;
    }

private:
    static void check(int rc) { if (rc != 0) throw std::runtime_error(std::string("libtrexhip: ") + trexhip_last_error()); }
    void release() {
        if (_d) (void)trexhip_device_free(_ctx, _d);
        _d = nullptr; _cap = 0;
    }
    void reserve(size_t n) {
        if (n <= _cap) return;
        release();
        check(trexhip_device_alloc(_ctx, n, reinterpret_cast<void**>(&_d)));
        _cap = n;
    }
    trexhip_ctx* _ctx;
    uint8_t* _d = nullptr;
    size_t _cap = 0;
};

}  // namespace track
