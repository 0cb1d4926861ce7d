// The record of trexhip_identify_prepare_device and its match rule (trex_amd/csrc/cnn_prepared.h), on the CPU.  Each argument names a check; the
// program prints "<check> ok" or "<check> FAILED: ..." per argument and returns the number of failures.
#include <cstdio>
#include <cstring>
#include <string>
#include "../../trex_amd/csrc/cnn_prepared.h"

using namespace trexhip;

static int failures = 0;
static void expect(const char* check, const bool ok, const char* what) {
    if (!ok) { std::printf("%s FAILED: %s\n", check, what); ++failures; }
}

static char buf_a[16], buf_b[16], stream_a, stream_b;

// a state with a record made from the reference call
static PreparedState prepared() {
    PreparedState s;
    s.weights_gen = 3; s.batch_gen = 7;
    s.set(s.make(buf_a, 1056, 3, 1 << 29, &stream_a));
    return s;
}
static PreparedKey same_call(const PreparedState& s) { return s.make(buf_a, 1056, 3, 1 << 29, &stream_a); }

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const std::string c = argv[i];
        const int before = failures;
        if (c == "match") {
            PreparedState s = prepared();
            expect(argv[i], s.valid, "a set record is valid");
            expect(argv[i], s.consume(same_call(s)), "the call it was made for finds it");
            PreparedState none;
            expect(argv[i], !none.consume(none.make(buf_a, 1056, 3, 1 << 29, &stream_a)), "no record, no match");
        } else if (c == "fields") {
            // every field differing in turn
            struct Case { const char* name; const void* crops; int n, mode, geom; const void* stream; int dw, db; } cases[] = {
                {"crops", buf_b, 1056, 3, 1 << 29, &stream_a, 0, 0},      {"crops + 1", buf_a + 1, 1056, 3, 1 << 29, &stream_a, 0, 0},
                {"n smaller", buf_a, 1055, 3, 1 << 29, &stream_a, 0, 0},  {"n larger", buf_a, 1057, 3, 1 << 29, &stream_a, 0, 0},
                {"mode", buf_a, 1056, 1, 1 << 29, &stream_a, 0, 0},       {"geom", buf_a, 1056, 3, 1 << 29 | 1 << 21, &stream_a, 0, 0},
                {"stream", buf_a, 1056, 3, 1 << 29, &stream_b, 0, 0},     {"null stream", buf_a, 1056, 3, 1 << 29, nullptr, 0, 0},
                {"weights generation", buf_a, 1056, 3, 1 << 29, &stream_a, 1, 0}, {"batch generation", buf_a, 1056, 3, 1 << 29, &stream_a, 0, 1},
            };
            for (const Case& k : cases) {
                PreparedState s = prepared();
                PreparedKey key = s.make(k.crops, k.n, k.mode, k.geom, k.stream);
                key.weights_gen += k.dw; key.batch_gen += k.db;
                expect(argv[i], !(key == s.key), k.name);
                expect(argv[i], !s.consume(key), k.name);
                expect(argv[i], !s.valid, "a mismatch takes the record as well");
                expect(argv[i], !s.consume(same_call(s)), "... so that the right call behind it runs its whole chain");
            }
        } else if (c == "one_shot") {
            PreparedState s = prepared();
            expect(argv[i], s.consume(same_call(s)), "first");
            expect(argv[i], !s.consume(same_call(s)), "consumed twice");
            s.set(same_call(s));
            s.set(s.make(buf_b, 100, 3, 0, &stream_b));                  // a second prepare replaces the first
            expect(argv[i], !s.consume(same_call(s)), "replaced");
            s.set(same_call(s)); s.set(same_call(s));
            expect(argv[i], s.consume(same_call(s)) && !s.valid, "prepared twice for the same call");
            // records made and records found, as trexhip_identify_prepare_stats reports them: 1 + 2 + 2 set, the first and the last found
            expect(argv[i], s.records == 5 && s.hits == 2, "counters");
        } else if (c == "dropped") {
            // each of the four events, then the call the record was made for: with the key it had, and with the key of a call made now
            for (int ev = 0; ev < 4; ++ev) {
                PreparedState s = prepared();
                const PreparedKey old = s.key;
                const uint64_t w0 = s.weights_gen, b0 = s.batch_gen;
                if (ev == 0) s.weights_loaded();
                if (ev == 1) s.precision_changed();
                if (ev == 2) s.batch_reallocated();
                if (ev == 3) s.closed();
                const char* names[] = {"weights loaded", "precision changed", "batch reallocated", "closed"};
                expect(argv[i], !s.valid, names[ev]);
                expect(argv[i], s.weights_gen == w0 + (ev == 0) && s.batch_gen == b0 + (ev == 2), "generations");
                PreparedState t = s;
                expect(argv[i], !s.consume(same_call(s)), names[ev]);
                expect(argv[i], !t.consume(old), names[ev]);
                // a record smuggled past the drop still cannot match a call made after a new generation began
                if (ev == 0 || ev == 2) {
                    PreparedState u = prepared();
                    if (ev == 0) ++u.weights_gen; else ++u.batch_gen;
                    expect(argv[i], !u.consume(same_call(u)), "an old generation's record");
                }
            }
        } else {
            std::printf("%s FAILED: unknown check\n", argv[i]);
            ++failures;
        }
        if (failures == before) std::printf("%s ok\n", argv[i]);
    }
    return failures;
}
