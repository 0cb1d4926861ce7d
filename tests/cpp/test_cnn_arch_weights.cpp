// The weight preparation of the identity networks v100 / v110 / v119 / v200 (trex_amd/csrc/cnn_weights.h) on the CPU: reads a weight blob, runs
// parse_arch_blob and every packer as arch_load (cnn_arch.hip) calls them, and writes each image as raw bytes into a directory
// (tests/test_cnn_arch_weights.py compares them with a numpy restatement).  A blob the parser refuses is reported as "refused <code> <error
// text>"; "v118_3 <code> <text>" is what parse_weight_blob, the trainer's parser, says to the same blob.  No device call is made.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "../../trex_amd/csrc/cnn_arch_plan.h"
#include "../../trex_amd/csrc/cnn_weights.h"

static std::string g_error;
namespace trexhip { void set_error(const std::string& msg) { g_error = msg; } }
using namespace trexhip;

static std::string g_dir;
template <class T>
static void dump(const std::string& name, const std::vector<T>& v) {
    std::ofstream f(g_dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s blob out_dir\n", argv[0]); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    g_dir = argv[2];
    WeightBlob old;
    const int orc = parse_weight_blob(blob.data(), blob.size(), "trexhip_trainer_create", &old);
    std::printf("v118_3 %d %s\n", orc, orc ? g_error.c_str() : "");
    ArchBlob wb;
    const int rc = parse_arch_blob(blob.data(), blob.size(), "trexhip_load_weights", &wb);
    if (rc != 0) { std::printf("refused %d %s\n", rc, g_error.c_str()); return 0; }
    std::printf("header %d %d %d %d %d id %d bytes %zu\n", wb.id, wb.classes, wb.W, wb.H, wb.CH, blob_arch_id(blob.data(), blob.size()),
                arch_blob_bytes(wb.id, wb.classes, wb.CH, wb.W, wb.H));
    if (reinterpret_cast<const char*>(wb.fc2b + wb.classes) != blob.data() + blob.size()) { std::printf("the tensors do not fill the blob\n"); return 1; }
    const ArchPlan p = arch_plan(wb.id, wb.W, wb.H, wb.CH);
    const ArchSpec& sp = *p.spec;
    const bool fold = sp.bn2d && !sp.bn_behind_pool;
    for (int i = 0; i < sp.n_conv; ++i) {
        const ArchLayerPlan& l = p.L[i];
        const std::string n = "c" + std::to_string(i + 1);
        const ArchConvImage im = i == 0 ? pack_arch_conv1(wb.conv[i], sp.conv[i].CO, wb.CH, l.taps, l.CO, fold)
                                        : pack_arch_conv(wb.conv[i], sp.conv[i].CO, sp.conv[i - 1].CO, l.taps, l.CO, l.CI, l.COB, fold);
        dump(n + "_w", im.w); dump(n + "_b", im.bias); dump(n + "_s", im.s); dump(n + "_t", im.t);
        if (i > 0) {
            dump(n + "_bf16", pack_arch_bf16x3(im.w, l.COB));
            const ScaledImage h = pack_arch_f16x2(im.w, l.COB);
            dump(n + "_f16", h.v);
            std::printf("inv %s_f16 %a\n", n.c_str(), (double)h.inv);
        }
    }
    const Folded f1 = pack_arch_fc1(wb.fc1w, wb.fc1b, sp.hidden, p.NH, sp.conv[sp.n_conv - 1].CO, p.Cf, sp.gap ? 1 : p.Hf * p.Wf);
    dump("fc1_w", f1.w); dump("fc1_b", f1.b);
    const Folded bn = pack_arch_bn1d(wb.bn1d, sp.hidden, p.NH);
    dump("head_s", bn.w); dump("head_t", bn.b);
    dump("fc2_t", pack_arch_fc2(wb.fc2w, wb.classes, sp.hidden));
    return 0;
}
