// Stand-alone driver of the stored-frame reader's host side (no GPU, no HIP runtime): trex_amd/csrc/pv_read.h (layout + bounds rules, the
// ones the device loader applies), trex_amd/csrc/pvfile.cpp (data section, LZO1X decoder) and the adapter's body writer
// (trex_amd/host/HipTrackFrames.h).  tests/test_pv_read.py builds it twice -- plain and with -fsanitize=address,undefined -- and compares
// what it prints with the oracle.
//   walk W H FILE             FILE = u32 count, count x {u32 length, bytes}: every entry is walked as one frame body.  Prints per frame
//                             "frame I malformed" or "frame I ok TS BLOBS LINES PIXELS", then per blob "blob OFF START_Y LINES PIXELS X0 Y0 X1 Y1 BID",
//                             its lines "line X0 X1 Y" and "pixels HEX"
//   section OFFSET DATA INDEX W H    trexhip_pv_read_frames on a data section (INDEX = u64 entries), then the walk of every body it returns
//   decompress LEN FILE       trexhip_lzo1x_decompress into LEN bytes: "ok N HEX" or "refused"
//   serialize IN OUT          IN = text: TS NBLOBS, per blob NLINES NPIXELS, NLINES x (Y X0 X1), NPIXELS values -> pv::Frame (stand-in) ->
//                             write_frame_body_v6 -> OUT
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "../../include/trexhip.h"
#include "../../trex_amd/csrc/pv_read.h"
#include "../../trex_amd/host/HipTrackFrames.h"

namespace trexhip {
static std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }
}

using namespace trexhip;

static std::vector<uint8_t> read_file(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Printer {
    struct Blob { uint64_t off; uint32_t start_y, lines, x0, y0, x1, y1, fx0, fx1; std::vector<uint32_t> l; std::vector<uint8_t> px; };
    std::vector<Blob> blobs;
    void blob(uint32_t, uint64_t off, uint32_t start_y, uint32_t lines) { blobs.push_back(Blob{off, start_y, lines, 0xffffu, start_y, 0u, start_y, 0u, 0u, {}, {}}); }
    void line(uint32_t x0, uint32_t x1, uint32_t y) {
        Blob& b = blobs.back();
        if (b.l.empty()) { b.fx0 = x0; b.fx1 = x1; }
        b.l.push_back(x0); b.l.push_back(x1); b.l.push_back(y);
        if (x0 < b.x0) b.x0 = x0;
        if (x1 > b.x1) b.x1 = x1;
        if (y > b.y1) b.y1 = y;
    }
    void pixels(const uint8_t* p, uint64_t n) { blobs.back().px.assign(p, p + n); }
};

// the bytes are copied into an allocation of exactly their size first: a read past the frame's end is one past a heap block (AddressSanitizer)
static void walk(int i, const uint8_t* bytes, size_t len, uint32_t W, uint32_t H) {
    uint8_t* body = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    if (len) std::memcpy(body, bytes, len);
    Printer pr;
    uint32_t lines = 0;
    uint64_t px = 0;
    if (!pvr::walk_frame(body, len, W, H, pr, &lines, &px)) std::printf("frame %d malformed\n", i);
    else {
        std::printf("frame %d ok %llu %zu %u %llu\n", i, (unsigned long long)pvr::frame_timestamp(body), pr.blobs.size(), lines, (unsigned long long)px);
        for (const Printer::Blob& b : pr.blobs) {
            std::printf("blob %llu %u %u %zu %u %u %u %u %u\n", (unsigned long long)b.off, b.start_y, b.lines, b.px.size(), b.x0, b.y0, b.x1, b.y1,
                        pvr::bid_of(b.fx0, b.fx1, b.start_y, b.lines));
            for (size_t j = 0; j + 2 < b.l.size(); j += 3) std::printf("line %u %u %u\n", b.l[j], b.l[j + 1], b.l[j + 2]);
            std::printf("pixels ");
            for (uint8_t p : b.px) std::printf("%02x", p);
            std::printf("\n");
        }
    }
    std::free(body);
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "walk" && argc == 5) {
        const uint32_t W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]);
        const std::vector<uint8_t> in = read_file(argv[4]);
        uint32_t count = 0;
        size_t o = 4;
        if (in.size() < 4) return 2;
        std::memcpy(&count, in.data(), 4);
        for (uint32_t i = 0; i < count; ++i) {
            uint32_t len = 0;
            if (o + 4 > in.size()) return 2;
            std::memcpy(&len, in.data() + o, 4); o += 4;
            if (o + len > in.size()) return 2;
            walk((int)i, in.data() + o, len, W, H);
            o += len;
        }
        return 0;
    }
    if (mode == "section" && argc == 7) {
        const uint64_t file_offset = std::strtoull(argv[2], nullptr, 10);
        const std::vector<uint8_t> data = read_file(argv[3]), idx_bytes = read_file(argv[4]);
        const uint32_t W = (uint32_t)std::atoi(argv[5]), H = (uint32_t)std::atoi(argv[6]);
        const int32_t n = (int32_t)(idx_bytes.size() / 8);
        std::vector<uint64_t> idx((size_t)n), off((size_t)n + 1);
        if (n) std::memcpy(idx.data(), idx_bytes.data(), (size_t)n * 8);
        size_t need = 0;
        // (the data in an allocation of exactly its size, as in walk())
        uint8_t* d = static_cast<uint8_t*>(std::malloc(data.size() ? data.size() : 1));
        if (!data.empty()) std::memcpy(d, data.data(), data.size());
        int rc = trexhip_pv_read_frames(d, data.size(), file_offset, idx.data(), n, nullptr, 0, off.data(), &need);
        if (rc == 0) {
            std::vector<uint8_t> bodies(need ? need : 1);
            rc = trexhip_pv_read_frames(d, data.size(), file_offset, idx.data(), n, bodies.data(), need, off.data(), &need);
            if (rc == 0) {
                // one byte less than needed is refused, not overrun
                std::vector<uint8_t> small(need > 1 ? need - 1 : 1);
                size_t got = 0;
                std::vector<uint64_t> off2((size_t)n + 1);
                if (need > 0 && trexhip_pv_read_frames(d, data.size(), file_offset, idx.data(), n, small.data(), need - 1, off2.data(), &got) == 0) { std::printf("short buffer accepted\n"); return 1; }
                for (int32_t f = 0; f < n; ++f) walk(f, bodies.data() + off[f], (size_t)(off[f + 1] - off[f]), W, H);
            }
        }
        std::free(d);
        if (rc != 0) std::printf("refused %d %s\n", rc, g_error.c_str());
        return 0;
    }
    if (mode == "decompress" && argc == 4) {
        const size_t cap = (size_t)std::strtoull(argv[2], nullptr, 10);
        const std::vector<uint8_t> in = read_file(argv[3]);
        uint8_t* src = static_cast<uint8_t*>(std::malloc(in.size() ? in.size() : 1));
        if (!in.empty()) std::memcpy(src, in.data(), in.size());
        uint8_t* dst = static_cast<uint8_t*>(std::malloc(cap ? cap : 1));
        size_t got = 0;
        if (trexhip_lzo1x_decompress(src, in.size(), dst, cap, &got) != 0) std::printf("refused\n");
        else {
            std::printf("ok %zu ", got);
            for (size_t i = 0; i < got; ++i) std::printf("%02x", dst[i]);
            std::printf("\n");
        }
        std::free(src); std::free(dst);
        return 0;
    }
    if (mode == "serialize" && argc == 4) {
        std::ifstream f(argv[2]);
        unsigned long long ts = 0;
        int nb = 0;
        f >> ts >> nb;
        pv::Frame frame;
        for (int b = 0; b < nb; ++b) {
            int nl = 0, np = 0;
            f >> nl >> np;
            auto lines = std::make_unique<std::vector<cmn::HorizontalLine>>();
            auto px = std::make_unique<cmn::PixelArray_t>();
            for (int j = 0; j < nl; ++j) { int y, x0, x1; f >> y >> x0 >> x1; lines->emplace_back((uint16_t)y, (uint16_t)x0, (uint16_t)x1); }
            for (int j = 0; j < np; ++j) { int v; f >> v; px->push_back((uint8_t)v); }
            frame.add_object(cmn::blob::Pair(std::move(lines), std::move(px)));
        }
        if (!f) { std::fprintf(stderr, "bad frame description\n"); return 2; }
        std::vector<uint8_t> out;
        track::write_frame_body_v6(frame, ts, out);
        std::ofstream o(argv[3], std::ios::binary);
        o.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)out.size());
        return 0;
    }
    std::fprintf(stderr, "usage: test_pv_read walk W H FILE | section OFFSET DATA INDEX W H | decompress LEN FILE | serialize IN OUT\n");
    return 2;
}
