// Holds the passes of TILE slots of the listed conv3 (trex_amd/csrc/cnn_skip3.h: Skip3TGeom, Skip3TXGeom, skip3t_add_run, skip3t_describe and
// skip3t_row_words, the row words of the pairs a pass touches) to a brute-force walk, tile pair by tile pair; tests/test_cnn_skip3t.py builds and runs it.
//   exhaust            every sequence of up to 4 runs of 1 .. 10 pairs, in both geometries, at two places in the batch (inside a block of 32 crops
//                      and across the edge of one) and with the runs at the top and at the bottom of their crops; prints "ok <sequences> <passes>"
//   count g len ...    the passes of geometry g (0 full width, 1 windowed) that the runs of one block make: "passes <n>"
#include "../../trex_amd/csrc/cnn_skip3.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace trexhip;

struct Run { int crop, q0, len, t0; };
struct Tile { int gp, place, crop, t0; };

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// the walker of the list kernels (cnn_skip_kernels.h: skip3_walk): a block's runs in order, the last pass flushed at the block's end
template <class T>
static std::vector<Skip3TPass> pack(const std::vector<Run>& runs) {
    std::vector<Skip3TPass> out;
    auto emit = [&](const int idx, const Skip3TPass& p) { CHECK(idx == (int)out.size(), "index %d", idx); out.push_back(p); };
    Skip3TPass p{};
    int passes = 0, blk = -1;
    for (const Run& r : runs) {
        if (r.crop / T::BLOCK != blk) { skip3t_flush(p, passes, emit); blk = r.crop / T::BLOCK; }
        skip3t_add_run<T>(p, passes, r.crop * T::PAIRS + r.q0, r.len, emit);
    }
    skip3t_flush(p, passes, emit);
    return out;
}

// the same count without the header: tile pairs in order, each into the open pass unless a rule closes that
template <class T>
static int brute(const std::vector<Run>& runs, const int maxp, const int nr) {
    int passes = 0, n = 0, nruns = 0, blk = -1, pairs = 0, rows = 0, last_run = -1, last_gp = -1;
    for (int r = 0; r < (int)runs.size(); ++r)
        for (int q = 0; q < runs[r].len; ++q)
            for (int pl = 0; pl < T::TPP; pl += 2) {
                const int gp = runs[r].crop * T::PAIRS + runs[r].q0 + q;
                const bool new_run = r != last_run, new_pair = new_run || gp != last_gp;
                bool close = n == 0 ? false : n == 64 || runs[r].crop / T::BLOCK != blk || (new_run && nruns == 2) || (new_pair && pairs == maxp);
                if (close || n == 0) {
                    if (n) ++passes;
                    n = 0; nruns = 0; pairs = 0; rows = 0; blk = runs[r].crop / T::BLOCK; last_run = -1; last_gp = -1;
                }
                if (r != last_run) { ++nruns; rows += 4; }
                if (r != last_run || gp != last_gp) { ++pairs; rows += 2; }
                last_run = r; last_gp = gp; n += 2;
                CHECK(rows <= nr + 4, "rows %d", rows);       // (rows: an upper bound, before the clip at the crop's edges)
            }
    return passes + (n > 0);
}

template <class T>
static int check_sequence(const std::vector<Run>& runs, const int total_crops) {
    using R = Skip3Reach;
    constexpr int BASE = T::ROW_WORDS - 1;
    std::vector<Tile> want;
    for (const Run& r : runs)
        for (int q = 0; q < r.len; ++q)
            for (int pl = 0; pl < T::TPP; ++pl) want.push_back({r.crop * T::PAIRS + r.q0 + q, pl, r.crop, r.t0});
    const std::vector<Skip3TPass> passes = pack<T>(runs);
    size_t at = 0;
    bool early = false;
    const long long total = (long long)total_crops * SkipGeom::V3_ROWS;
    const SkipRows every{0, SkipGeom::V3_ROWS - 1};
    for (const Skip3TPass& p : passes) {
        const int cap = T::MB;
        CHECK(p.n > 0 && p.n <= cap && p.n % 2 == 0 && p.o % 2 == 0 && p.o >= 0 && p.o <= T::TPP - 2, "n %d o %d", p.n, p.o);
        CHECK(p.runs >= 1 && p.runs <= T::RUNS, "runs %d", p.runs);
        CHECK(!early || p.o == 0, "a pass behind an early close begins %d tiles into a pair", p.o);
        const Skip3Pass pp = skip3t_pairs(p);
        CHECK(pp.n <= T::MAXP, "pairs %d", pp.n);
        const int first_crop = p.gp0[0] / T::PAIRS, last_crop = (p.runs > 1 ? p.gp0[1] : p.gp0[0]) / T::PAIRS;
        CHECK(first_crop / T::BLOCK == last_crop / T::BLOCK, "crops %d and %d in one pass", first_crop, last_crop);
        int t0a = 0, t0b = 0;
        for (const Run& r : runs) { if (r.crop == first_crop) t0a = r.t0; if (r.crop == last_crop) t0b = r.t0; }
        int d[T::DESC];
        skip3t_describe<T>(p, d, t0a, t0b);
        unsigned w[T::ROW_WORDS];
        skip3t_row_words<T>(pp, every, every, total, w, t0a, t0b);
        CHECK(d[S3_ROWS] <= T::NR && d[S3_ROWS] > 0, "rows %d", d[S3_ROWS]);
        CHECK((d[S3_TILES] & S3_O_MASK) == p.o && d[S3_TILES] >> S3_COUNT_SHIFT == p.n, "word S3_TILES %d", d[S3_TILES]);
        CHECK(d[S3_GP0] == p.gp0[0] && d[S3_GP0] + d[S3_SPAN] - 1 == want[at + p.n - 1].gp, "the act3 range %d + %d", d[S3_GP0], d[S3_SPAN]);
        for (int t = 0; t < p.n; ++t, ++at) {
            CHECK(at < want.size(), "more tiles than listed");
            const Tile& x = want[at];
            const int slot = (p.o + t) / T::TPP, place = (p.o + t) % T::TPP;
            CHECK(slot < T::SLOTS, "slot %d", slot);
            const int e = d[S3_SLOT + slot];
            CHECK(((unsigned)e >> 16) != (unsigned)S3_IDLE && d[S3_GP0] + (e >> 16) == x.gp && place == x.place, "tile %d of the pass: pair %d place %d, wanted %d %d", t, d[S3_GP0] + (e >> 16), place, x.gp, x.place);
            CHECK(((e >> 8) & S3_Q_MASK) == x.gp % T::PAIRS && ((e >> S3_T0_SHIFT) & S3_T0_MASK) == x.t0, "q %d t0 %d", (e >> 8) & S3_Q_MASK, (e >> S3_T0_SHIFT) & S3_T0_MASK);
            // the row slot of the pair's even conv row, and the five + one V3 rows around it that its taps read: each from its own row of V3
            const int rs = e & 0xff, q = x.gp % T::PAIRS;
            for (int dy = -T::HALO; dy < SkipGeom::POOL + T::HALO; ++dy) {
                const int y = SkipGeom::POOL * q + dy, i = rs - 1 + dy;
                if (y < 0 || y >= SkipGeom::V3_ROWS) continue;
                CHECK(i >= 0 && i < d[S3_ROWS], "row slot %d of %d", i + 1, d[S3_ROWS]);
                const unsigned off = w[i] + ((unsigned)i << R::ROW_SHIFT);
                const long long row = (long long)w[BASE] + off / R::ROWB;
                CHECK(row == SkipGeom::V3_ROWS + (long long)x.crop * SkipGeom::V3_ROWS + y && (int)(off % R::ROWB) == x.t0 * R::TILEB,
                      "row slot %d holds row %lld + %u bytes, wanted crop %d row %d", i + 1, row, off % R::ROWB, x.crop, y);
            }
        }
        // the lanes of the tile slots behind the pass's tiles look at slots of the descriptor, too
        CHECK((p.o + T::MB - 1) / T::TPP < T::SLOTS, "slot of the last lane");
        for (int s = pp.n; s < T::SLOTS; ++s) CHECK(((unsigned)d[S3_SLOT + s] >> 16) == (unsigned)S3_IDLE, "slot %d is not idle", s);
        for (int i = d[S3_ROWS]; i < BASE; ++i) CHECK(w[i] + ((unsigned)i << R::ROW_SHIFT) >= R::NUM_RECORDS, "row word %d behind the pass's rows", i);
        early = p.n < cap;
    }
    CHECK(at == want.size(), "%zu of %zu tiles in passes", at, want.size());
    const int b = brute<T>(runs, T::MAXP, T::NR);
    CHECK((int)passes.size() == b, "%zu passes, brute force %d", passes.size(), b);
    return (int)passes.size();
}

template <class T>
static void exhaust(long long& sequences, long long& passes) {
    constexpr bool WIN = T::TILES != Skip3Geom::TILES;
    for (int n = 1; n <= 4; ++n) {
        int len[4] = {1, 1, 1, 1};
        for (;;) {
            for (int place = 0; place < 2; ++place)          // crops 3 .. or 30 ..: the edge of a block lies behind the second one
                for (int top = 0; top < 2; ++top) {
                    std::vector<Run> runs;
                    for (int k = 0; k < n; ++k) {
                        const int crop = (place ? 30 : 3) + k;
                        runs.push_back({crop, top ? 0 : T::PAIRS - len[k], len[k], WIN ? crop % 3 : 0});
                    }
                    passes += check_sequence<T>(runs, 40);
                    ++sequences;
                }
            int k = 0;
            while (k < n && ++len[k] > T::PAIRS) len[k++] = 1;
            if (k == n) break;
        }
    }
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "exhaust")) {
        long long sequences = 0, passes = 0;
        exhaust<Skip3TGeom>(sequences, passes);
        exhaust<Skip3TXGeom>(sequences, passes);
        std::printf("ok %lld %lld\n", sequences, passes);
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "count")) {
        std::vector<Run> runs;
        for (int i = 3; i < argc; ++i) {
            const int len = std::atoi(argv[i]);
            if (len < 1 || len > Skip3Geom::PAIRS || i - 3 >= Skip3Geom::BLOCK) { std::fprintf(stderr, "bad run: %s\n", argv[i]); return 2; }
            runs.push_back({i - 3, 0, len, 0});
        }
        const int n = std::atoi(argv[2]) ? (int)pack<Skip3TXGeom>(runs).size() : (int)pack<Skip3TGeom>(runs).size();
        std::printf("passes %d\n", n);
        return 0;
    }
    std::fprintf(stderr, "usage: exhaust | count g len ...\n");
    return 2;
}
