// cnn_prepared.h -- the record trexhip_identify_prepare_device leaves for the next trexhip_identify_device on its context, and the rule by which
// that call may skip the launches the record stands for (the role-split chain's preparation: launch_skip_prep and k_act3_fill, cnn.hip).
// No device code and no HIP: tests/cpp/test_cnn_prepared.cpp holds it to the rule stated here.
//
//   * One record per context.  A prepare call replaces it; a call that launched nothing (another chain, another mode, the captured-graph path)
//     leaves none.
//   * The next forward pass of the context TAKES the record whatever its arguments are (one-shot): it skips the prepared launches only if every
//     field equals what the pass itself would have prepared from -- crops pointer, n, precision mode, TREXHIP_CONV_GEOM value, stream, and the
//     generations of the loaded weights and of the batch allocation the prepared words and lists live in.  Anything else runs the whole chain,
//     which rewrites every prepared word (none of them accumulates across calls).
//   * Loading weights, changing the precision mode, reallocating the batch buffers and closing the context drop the record; the first and the
//     third also start a new generation, so that a record made before them can never match again.
// What the record cannot see is the caller's: the crops' bytes must not change between the prepare call and the identify call.
#pragma once
#include <cstdint>

namespace trexhip {

struct PreparedKey {
    const void* crops;
    int n, mode, geom;
    const void* stream;
    uint64_t weights_gen, batch_gen;
};
inline bool operator==(const PreparedKey& a, const PreparedKey& b) {
    return a.crops == b.crops && a.n == b.n && a.mode == b.mode && a.geom == b.geom && a.stream == b.stream && a.weights_gen == b.weights_gen &&
           a.batch_gen == b.batch_gen;
}

struct PreparedState {
    bool valid = false;
    PreparedKey key{};
    uint64_t weights_gen = 0, batch_gen = 0;      // of the context, not of the record
    uint32_t records = 0, hits = 0;               // records made, records a forward pass found its launches done by (trexhip_identify_prepare_stats)

    // the key of a call made now
    PreparedKey make(const void* crops, const int n, const int mode, const int geom, const void* stream) const {
        return {crops, n, mode, geom, stream, weights_gen, batch_gen};
    }
    void set(const PreparedKey& k) { key = k; valid = true; ++records; }
    void drop() { valid = false; }
    // a forward pass with key k: were its preparation's launches made already?  The record is gone either way
    bool consume(const PreparedKey& k) {
        const bool hit = valid && key == k;
        valid = false;
        hits += hit ? 1u : 0u;
        return hit;
    }
    void weights_loaded() { ++weights_gen; drop(); }
    void precision_changed() { drop(); }
    void batch_reallocated() { ++batch_gen; drop(); }
    void closed() { drop(); }
};

}  // namespace trexhip
