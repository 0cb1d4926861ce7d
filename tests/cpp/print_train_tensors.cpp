// Prints the tensor table of a trainer (trex_amd/csrc/train_tensors.h), one line per argument:
//   net,W,H,CH,classes   ->   name=value pairs; net = 0 V118_3, 1 v100, 2 v110, 3 the category network
// Lists are comma separated.  order / cnt / isz / off run over the state_dict positions; slots / total / keep_off / keep_row / buffers are the
// table's own; outside = elements that to_internal puts outside [0, isz), twice = elements that land where another of the same tensor already
// has (both walk every element of every tensor).  tests/test_train_tensors.py holds the lines to trex_amd/weights.py and to literals.
#include "../../trex_amd/csrc/train_tensors.h"
#include <cstdio>
#include <vector>

using namespace trexhip;

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        int net, W, H, CH, classes;
        if (std::sscanf(argv[a], "%d,%d,%d,%d,%d", &net, &W, &H, &CH, &classes) != 5 || net < 0 || net > 3) {
            std::fprintf(stderr, "bad case: %s\n", argv[a]);
            return 2;
        }
        const TrainTensors t = train_tensors((TrainNet)net, W, H, CH, classes);
        size_t outside = 0, twice = 0;
        for (int k = 0; k < t.n_tensors; ++k) {
            const int slot = t.order[k];
            std::vector<char> seen(t.isz[slot], 0);
            for (size_t i = 0; i < t.cnt[slot]; ++i) {
                const size_t at = t.to_internal(slot, i);
                if (at >= seen.size()) { ++outside; continue; }
                twice += seen[at];
                seen[at] = 1;
            }
        }
        std::printf("taps=%d slots=%d total=%zu keep_row=%zu outside=%zu twice=%zu", t.taps, t.n_slots, t.total, t.keep_row, outside, twice);
        const char* names[4] = {"order", "cnt", "isz", "off"};
        for (int f = 0; f < 4; ++f) {
            std::printf(" %s=", names[f]);
            for (int k = 0; k < t.n_tensors; ++k) {
                const int slot = t.order[k];
                std::printf("%s%zu", k ? "," : "", f == 0 ? (size_t)slot : f == 1 ? t.cnt[slot] : f == 2 ? t.isz[slot] : t.off[slot]);
            }
        }
        std::printf(" keep_off=%zu,%zu,%zu,%zu buffers=", t.keep_off[0], t.keep_off[1], t.keep_off[2], t.keep_off[3]);
        for (int k = 0; k < t.n_buffers; ++k) std::printf("%s%d", k ? "," : "", t.buffers[k]);
        std::printf("\n");
    }
    return 0;
}
