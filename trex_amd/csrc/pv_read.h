// pv_read.h -- the layout of a V_6 frame body and every bounds rule of reading one, for the host and the device.
//
// What pv::Frame::read_from accepts for file version V_6 (ProcessedVideo/pv.cpp:296-420; LegacyShortHorizontalLine pv.h:17-52), i.e. what
// pack.hip writes (layout comment there, :3-11):
//     u8  compression_flag = 0      u64 timestamp      u16 n
//     n x { u16 start_y, u16 mask_size, mask_size x {u16 x0, u16 (x1 << 1) | eol}, one byte per pixel }
// A line's y is start_y plus the number of eol bits in front of it.  All fields are assembled from bytes: bodies sit at arbitrary offsets.
//
// A frame is MALFORMED when
//   - it is shorter than 11 bytes or its flag byte is not 0                                                  frame_head_ok
//   - a blob header, its 4 x mask_size line bytes or its pixel bytes would pass the frame's end (the end
//     comes from the offsets, never from the content), or mask_size == 0                                     read_blob_head, pixels_fit
//   - x0 > x1, x1 >= width, y >= height, or a line does not start to the right of the previous line of
//     its row (pv.cpp:505-508; the bisections downstream need strictly (y, x0)-sorted lines)                 line_ok
//   - bytes are left over behind the last blob                                                               frame_end_ok
// No HIP runtime calls in here: the file compiles as plain C++ (hipcc -x c++, g++) and inside kernels.  The device loader (unpack.hip)
// applies the per-line rules with 64 lanes at once; walk_frame below applies the same functions one line at a time (host reader, tests).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define PVR_FN __host__ __device__ inline
#else
#define PVR_FN inline
#endif

namespace trexhip {
namespace pvr {

enum : uint32_t { FRAME_HEAD = 11u, BLOB_HEAD = 4u, LINE_BYTES = 4u };
static constexpr uint64_t MAX_FRAME_BYTES = 0xffffffffull;       // a frame is below 4 GB (pv.cpp:726): counts and offsets inside one fit 32 bits

struct Line { uint32_t x0, x1, eol; };
struct BlobHead { uint32_t start_y, mask_size; };

PVR_FN uint32_t get16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
PVR_FN uint64_t get64(const uint8_t* p) { uint64_t v = 0; for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k); return v; }

// the frame's own bytes are body[0 .. len)
PVR_FN bool frame_head_ok(const uint8_t* body, uint64_t len) { return len >= FRAME_HEAD && len <= MAX_FRAME_BYTES && body[0] == 0; }
PVR_FN uint64_t frame_timestamp(const uint8_t* body) { return get64(body + 1); }
PVR_FN uint32_t frame_blobs(const uint8_t* body) { return get16(body + 9); }

// blob header at byte o of the frame; false: the header or the blob's line bytes pass the frame's end, or the blob has no lines
PVR_FN bool read_blob_head(const uint8_t* body, uint64_t len, uint64_t o, BlobHead& h) {
    if (o + BLOB_HEAD > len) return false;
    h.start_y = get16(body + o); h.mask_size = get16(body + o + 2);
    return h.mask_size != 0 && o + BLOB_HEAD + (uint64_t)LINE_BYTES * h.mask_size <= len;
}
PVR_FN Line read_line(const uint8_t* p) {
    const uint32_t w = get16(p + 2);
    Line l; l.x0 = get16(p); l.x1 = (w & 0xfffeu) >> 1; l.eol = w & 1u;
    return l;
}
// y: the line's row; new_row: it is the first line of its row inside the blob; prev_x1: x1 of the line in front of it (when !new_row)
PVR_FN bool line_ok(const Line& l, uint32_t y, bool new_row, uint32_t prev_x1, uint32_t width, uint32_t height) {
    return l.x0 <= l.x1 && l.x1 < width && y < height && (new_row || l.x0 > prev_x1);
}
PVR_FN uint32_t line_pixels(const Line& l) { return l.x1 - l.x0 + 1u; }
// pixel bytes [o, o + n_pixels) of the frame
PVR_FN bool pixels_fit(uint64_t o, uint64_t n_pixels, uint64_t len) { return o + n_pixels <= len; }
PVR_FN bool frame_end_ok(uint64_t o, uint64_t len) { return o == len; }

// pv::bid (commons): 13/13/6-bit hash of a blob's first line and its number of lines
PVR_FN uint32_t bid_of(uint32_t x0, uint32_t x1, uint32_t y, uint32_t n_lines) {
    uint32_t x = x0 + (x1 - x0 + 1u) / 2u;
    if (x > 8191u) x = 8191u;
    if (y > 8191u) y = 8191u;
    const uint32_t n = n_lines < 1u ? 1u : (n_lines > 63u ? 63u : n_lines);
    return (x << 19) | (y << 6) | n;
}

// One frame, line by line.  The visitor sees only what passed every rule in front of it:
//   v.blob(index, byte offset of the blob header, start_y, mask_size)      v.line(x0, x1, y)
//   v.pixels(pointer to the blob's pixel bytes, their number)              -- after the blob's lines
// Returns false for a malformed frame (the visitor may have seen its leading part); *n_lines / *n_pixels: totals of a good frame.
template <class Visitor>
PVR_FN bool walk_frame(const uint8_t* body, uint64_t len, uint32_t width, uint32_t height, Visitor& v, uint32_t* n_lines, uint64_t* n_pixels) {
    if (!frame_head_ok(body, len)) return false;
    const uint32_t n = frame_blobs(body);
    uint64_t o = FRAME_HEAD, total_px = 0;
    uint32_t total_lines = 0;
    for (uint32_t b = 0; b < n; ++b) {
        BlobHead h;
        if (!read_blob_head(body, len, o, h)) return false;
        v.blob(b, o, h.start_y, h.mask_size);
        uint32_t y = h.start_y, prev_x1 = 0;
        bool new_row = true;
        uint64_t px = 0;
        for (uint32_t j = 0; j < h.mask_size; ++j) {
            const Line l = read_line(body + o + BLOB_HEAD + (uint64_t)LINE_BYTES * j);
            if (!line_ok(l, y, new_row, prev_x1, width, height)) return false;
            v.line(l.x0, l.x1, y);
            px += line_pixels(l);
            prev_x1 = l.x1; new_row = l.eol != 0;
            y += l.eol;
        }
        o += BLOB_HEAD + (uint64_t)LINE_BYTES * h.mask_size;
        if (!pixels_fit(o, px, len)) return false;
        v.pixels(body + o, px);
        o += px; total_px += px; total_lines += h.mask_size;
    }
    if (!frame_end_ok(o, len)) return false;
    if (n_lines) *n_lines = total_lines;
    if (n_pixels) *n_pixels = total_px;
    return true;
}

// Bytes of the uncompressed frame that starts at data[0] when nothing but `avail` bounds it (a stored data section keeps no size for
// a frame of flag 0: its extent is the chain of its blob sizes).  Only the rules that the chain needs are applied here -- the full set
// runs when the frame is loaded.  false: the chain leaves `avail`.
PVR_FN bool frame_extent(const uint8_t* data, uint64_t avail, uint64_t* bytes) {
    if (avail < FRAME_HEAD || data[0] != 0) return false;
    const uint32_t n = frame_blobs(data);
    uint64_t o = FRAME_HEAD;
    for (uint32_t b = 0; b < n; ++b) {
        BlobHead h;
        if (!read_blob_head(data, avail, o, h)) return false;
        uint64_t px = 0;
        for (uint32_t j = 0; j < h.mask_size; ++j) {
            const Line l = read_line(data + o + BLOB_HEAD + (uint64_t)LINE_BYTES * j);
            if (l.x0 > l.x1) return false;
            px += line_pixels(l);
        }
        o += BLOB_HEAD + (uint64_t)LINE_BYTES * h.mask_size;
        if (!pixels_fit(o, px, avail)) return false;
        o += px;
    }
    if (o > MAX_FRAME_BYTES) return false;
    *bytes = o;
    return true;
}

}  // namespace pvr
}  // namespace trexhip
