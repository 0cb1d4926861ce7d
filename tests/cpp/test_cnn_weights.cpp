// The weight-preparation unit of the identity network (trex_amd/csrc/cnn_weights.h) on the CPU: reads a weight blob, runs the parser and
// every packer and writes each image as raw bytes into a directory (tests/test_cnn_weights.py compares them with a numpy restatement).
// A blob the parser refuses is reported as "refused <code> <error text>".  No device call is made.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "../../trex_amd/csrc/cnn_weights.h"

static std::string g_error;
namespace trexhip { void set_error(const std::string& msg) { g_error = msg; } }
using namespace trexhip;

static std::string g_dir;
template <class T>
static void dump(const char* name, const std::vector<T>& v) {
    std::ofstream f(g_dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}
static void dump(const char* name, const Folded& f) { dump((std::string(name) + "_w").c_str(), f.w); dump((std::string(name) + "_b").c_str(), f.b); }
static void dump(const char* name, const ScaledImage& im) { dump(name, im.v); std::printf("inv %s %a\n", name, (double)im.inv); }

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s blob out_dir\n", argv[0]); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    g_dir = argv[2];
    WeightBlob wb;
    const int rc = parse_weight_blob(blob.data(), blob.size(), "trexhip_load_weights", &wb);
    if (rc != 0) { std::printf("refused %d %s\n", rc, g_error.c_str()); return 0; }
    std::printf("header %d %d %d %d\n", wb.classes, wb.W, wb.H, wb.CH);
    size_t at = 32;
    for (int k = 0; k < T_COUNT; ++k) {
        if (reinterpret_cast<const char*>(wb.t[k]) != blob.data() + at) { std::printf("tensor %d is misplaced\n", k); return 1; }
        at += 4 * weight_tensor_count(k, wb.classes, wb.CH, wb.W, wb.H);
    }
    if (at != blob.size() || at != weight_blob_bytes(wb.classes, wb.CH, wb.W, wb.H)) { std::printf("the tensors do not fill the blob\n"); return 1; }

    const Folded c1 = fold_conv1(&wb.t[T_C1W], wb.CH);
    dump("c1", c1);
    dump("c1_frags", pack_conv1_frags(c1.w, wb.CH));
    const Folded c2 = fold_conv(&wb.t[T_C2W], 64, 16, 16);
    dump("c2", c2);
    dump("c2_bf16", pack_bf16x3(c2.w, 16, 64));
    dump("c2_f16", pack_f16x2(c2.w, 16, 64));
    dump("c2_wino", pack_wino_f16(c2.w, 16, 64));
    const Folded c3 = fold_conv(&wb.t[T_C3W], 128, 64, 16);
    dump("c3", c3);
    dump("c3_bf16", pack_bf16x3(c3.w, 64, 128));
    dump("c3_f16", pack_f16x2(c3.w, 64, 128));
    dump("c3_wino", pack_wino_f16(c3.w, 64, 128));
    dump("c3x32", fold_conv(&wb.t[T_C3W], 128, 64, 32));
    const Folded f1 = pack_fc1(wb.t[T_F1W], wb.t[T_F1B], wb.W, wb.H);
    dump("fc1", f1);
    dump("fc1_f16", pack_fc1_f16(f1.w));
    dump("fc2_t", pack_fc2(wb.t[T_F2W], wb.classes));
    return 0;
}
