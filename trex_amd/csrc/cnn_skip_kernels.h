// cnn_skip_kernels.h -- the per-call preparation that lets the role-split chain leave out what is background: the passes of k_conv12_rs whose
// crop rows are all zero (the rule: cnn_skip.h), the tile columns a crop's blob does not reach (cnn_skipx.h), the row pairs of conv3 and the
// (crop, plane) rows of fc1 that read no blob (cnn_skip3.h).  Included by cnn.hip inside namespace trexhip.  Small kernels on the forward pass's
// stream, no host read between them; the words they leave in Net::d_skip: cnn_skip_words.h.  In the order they run (launch_skip_prep):
//   k_crop_bands   first / last non-zero row of every crop (it looks at the bytes, not at how the crop was made), and, where crops can have
//                  windows (`cols` not null), the first / last non-zero column
//   k_pass_count   thread i: pass i and crop i.  Per SKIP_LB of them: full-width passes, passes the row rule lists, windowed passes, windowed crops,
//                  and, where the windowed instance leaves out background rows (`bgrows`), the V2 rows those passes read and the rows made of them
//   k_pass_list    order-preserving compaction into the lists k_conv12_rs walks: the aligned full-width passes that a crop WITHOUT a window needs,
//                  and the windowed passes of the crops that have one, beside each of these the V2 rows of its crop that are made at all
//                  (skipx_v2_rows; every row without `bgrows`); their lengths, the entry behind the end of each, the windowed instance's
//                  ticket counter zeroed, and SK_LEN / SK_NPASS / SK_FILLED by the row rule alone.  `cols` null: no crop has a window -- the
//                  full-width list is the row rule's, and neither the windowed list nor the SKX_* words are touched
//   k_pair_count   (listed conv3) listed passes per thread and passes and pairs per workgroup; a thread packs the row pairs of Skip3Geom::BLOCK
//                  consecutive crops -- where crops can have windows of conv3 tiles (`cols` not null; skip3_window), those of the crops with one
//                  into windowed passes (Skip3XGeom: 10 pairs), the others' into full-width passes (6 pairs), in one walk.  TILED: the lists the
//                  kernel walks are passes of tile slots (Skip3TXGeom, Skip3TGeom: up to 64 consecutive tiles); the passes of pair slots are still
//                  counted, by two more groups of threads, for the counters and for the choice of the form
//   k_pair_list    the passes of both lists in order, each as its two runs, the counters, the windowed instance's ticket counter zeroed, and the
//                  word that names the form of conv3 that runs (SK3_USE: the passes of both lists together against the dense kernel's)
//   k_fc1_list     (listed fc1) a workgroup per split-K plane: the crops whose pair the plane has to compute, in order, and how many they are
//   k_v3_fill      row by row: a V3 row that nobody computes -- its crop has no window over it and its aligned pass is not on the full-width
//                  list -- copied from the V3 image of an all-zero crop (Net::v3e, made at load).  For the dense conv3 only: where the listed
//                  form runs and takes those rows from the image itself (`direct`), it reads SK3_USE and returns at once
// and behind conv1+conv2:
//   k_act3_fill    a thread per pass of either list: the runs made into the descriptor the kernel reads (in place) and the sources of its rows; then
//                  a wave per crop: the act3 row pairs that are NOT listed, copied from the act3 of an all-zero crop (Net::act3e, made at load) --
//                  counted only, where the listed fc1 runs: it never reads them --, and of the LISTED pairs of a crop with a window the 4 pooled
//                  columns outside it, copied always
#pragma once

static constexpr int SKIP_LB = 1024;      // passes / crops per block of the count / list kernels (one per thread)
static constexpr int SKIP_PAD = 1;        // one entry behind the last one: k_conv12_rs clamps every read behind the list's end to it (RS_LIST)
static constexpr int SKIP_NCNT = 6;       // words per block that k_pass_count leaves for k_pass_list
static constexpr int SKIP_FILL_TB = 256;  // V3 rows per block of the fill kernel (one per thread)

// one wave per crop: 400 x 16 bytes, unit i lies in row i / 5
// cols (may be null): the first / last non-zero COLUMN as well (cnn_skipx.h), from the same registers
__global__ __launch_bounds__(256) void k_crop_bands(const uint8_t* __restrict__ crops, const int n, int2* __restrict__ bands, int2* __restrict__ cols) {
    using G = SkipGeom;
    constexpr int UPR = 80 / 16, UNITS = G::CROP_ROWS * UPR;
    const int lane = threadIdx.x & 63, crop = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (crop >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(crops + (size_t)crop * (G::CROP_ROWS * 80));
    uint4 px[(UNITS + 63) / 64];
#pragma unroll
    for (int k = 0; k < (UNITS + 63) / 64; ++k) {
        const int i = lane + 64 * k;
        px[k] = i < UNITS ? src[i] : make_uint4(0, 0, 0, 0);
    }
    int y0 = G::CROP_ROWS, y1 = -1;
#pragma unroll
    for (int k = 0; k < (UNITS + 63) / 64; ++k) {
        if (px[k].x | px[k].y | px[k].z | px[k].w) {
            const int row = (lane + 64 * k) / UPR;
            y0 = row < y0 ? row : y0;
            y1 = row > y1 ? row : y1;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_xor(y0, d), b = __shfl_xor(y1, d);
        y0 = a < y0 ? a : y0;
        y1 = b > y1 ? b : y1;
    }
    if (lane == 0) bands[crop] = make_int2(y0, y1);
    if (cols) {                                                          // wave-uniform
        int x0 = 80, x1 = -1;
#pragma unroll
        for (int k = 0; k < (UNITS + 63) / 64; ++k) {
            const int c0 = ((lane + 64 * k) % UPR) * 16;
            const uint32_t w4[4] = {px[k].x, px[k].y, px[k].z, px[k].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (w4[j]) {                                             // byte b of the word is column c0 + 4 j + b
                    const int a = c0 + 4 * j + ((__ffs((int)w4[j]) - 1) >> 3), b = c0 + 4 * j + ((31 - __clz((int)w4[j])) >> 3);
                    x0 = a < x0 ? a : x0;
                    x1 = b > x1 ? b : x1;
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int a = __shfl_xor(x0, d), b = __shfl_xor(x1, d);
            x0 = a < x0 ? a : x0;
            x1 = b > x1 ? b : x1;
        }
        if (lane == 0) cols[crop] = make_int2(x0, x1);
    }
}

struct SkipBandsOf {
    const int2* bands;
    __host__ __device__ SkipBand operator()(const int crop) const { const int2 b = bands[crop]; return {b.x, b.y}; }
};
__device__ __forceinline__ bool skip_needed(const int p, const int total_pairs, const int2* __restrict__ bands, const bool all) {
    return all || skip_pass_needed(p, total_pairs, SkipBandsOf{bands});
}
// a crop's window (cnn_skipx.h); a crop without a blob has a window and no pass.  cols null: no crop has one
struct SkipXWinOf {
    const int2* cols; bool all;
    __host__ __device__ int operator()(const int crop) const {
        if (!cols) return -1;
        const int2 c = cols[crop];
        return skipx_window({c.x, c.y}, all);
    }
};
// thread i of the grid: pass i of the batch (full width: is it needed by a crop without a window; and by the row rule alone, for the counters)
// and crop i (its windowed passes).  counts[SKIP_NCNT b ..]: full-width passes, aligned needed passes, windowed passes, windowed crops of block
// b; the V2 rows its windowed passes read -- a crop's passes taken as one run, as they are wherever no ticket ends inside the crop: the rows
// rs_v2_rows gives for its needed V3 rows -- and the rows of those that are made (both 0 without `bgrows`)
struct SkipXItem { bool full, need; int wpasses, t0; SkipRows rows; SkipV2 v2; int v2_read, v2_made; };
__device__ __forceinline__ SkipXItem skipx_item(const int i, const int n, const int2* __restrict__ bands, const int2* __restrict__ cols, const bool all,
                                                const bool bgrows) {
    const int total_pairs = n * SkipGeom::V3_ROWS, n_pass = (total_pairs + SkipGeom::RPP - 1) / SkipGeom::RPP;
    const bool none = all || !cols;      // no crop has a window: a pass is on the full-width list where the row rule lists it (uniform across the grid)
    SkipXItem it{false, false, 0, -1, {1, 0}, SKIPX_V2_ALL, 0, 0};
    if (i < n_pass) {
        it.need = skip_needed(i, total_pairs, bands, all);
        it.full = it.need && (none || skipx_full_needed(i, total_pairs, SkipBandsOf{bands}, SkipXWinOf{cols, all}));
    }
    if (i < n) {
        it.t0 = SkipXWinOf{cols, all}(i);
        const int2 b = bands[i];
        it.rows = skip_rows({b.x, b.y});
        it.wpasses = it.t0 >= 0 ? skipx_passes(it.rows) : 0;
        if (bgrows && it.wpasses) {
            it.v2 = skipx_v2_rows({b.x, b.y});
            const RsRound r = rs_round(false, 0, it.rows.lo, it.rows.hi, true, it.v2, SkipXGeom::CHUNK);      // (rows of the crop: crop 0 of a batch)
            it.v2_read = r.hi - r.lo;
            it.v2_made = r.chi - r.clo;
        }
    }
    return it;
}
__global__ __launch_bounds__(SKIP_LB) void k_pass_count(const int2* __restrict__ bands, const int2* __restrict__ cols, const int n,
                                                        const uint32_t* __restrict__ words, uint32_t* __restrict__ counts, const int bgrows) {
    __shared__ uint32_t s_cnt[SKIP_NCNT];
    if (threadIdx.x < SKIP_NCNT) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const SkipXItem it = skipx_item(blockIdx.x * SKIP_LB + threadIdx.x, n, bands, cols, words[SK_EMPTY_RANGE] != 0, bgrows != 0);
    uint32_t v[SKIP_NCNT] = {it.full ? 1u : 0u, it.need ? 1u : 0u, (uint32_t)it.wpasses, it.wpasses ? 1u : 0u, (uint32_t)it.v2_read, (uint32_t)it.v2_made};
#pragma unroll
    for (int k = 0; k < SKIP_NCNT; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d);
        if ((threadIdx.x & 63) == 0 && v[k]) atomicAdd(&s_cnt[k], v[k]);
    }
    __syncthreads();
    if (threadIdx.x < SKIP_NCNT) counts[blockIdx.x * SKIP_NCNT + threadIdx.x] = s_cnt[threadIdx.x];
}
__global__ __launch_bounds__(SKIP_LB) void k_pass_list(const int2* __restrict__ bands, const int2* __restrict__ cols, const int n,
                                                       uint32_t* __restrict__ words, const uint32_t* __restrict__ counts, int* __restrict__ list,
                                                       int* __restrict__ wlist, int* __restrict__ wrows, const int bgrows) {
    __shared__ uint32_t s_base[SKIP_NCNT], s_wave[2][SKIP_LB / 64];
    const int total_pairs = n * SkipGeom::V3_ROWS, n_pass = (total_pairs + SkipGeom::RPP - 1) / SkipGeom::RPP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * SKIP_LB + tid;
    if (tid < SKIP_NCNT) s_base[tid] = 0;
    __syncthreads();
    // what the blocks in front of this one counted
    uint32_t part[SKIP_NCNT] = {0, 0, 0, 0, 0, 0};
    for (int b = tid; b < (int)blockIdx.x; b += SKIP_LB) {
#pragma unroll
        for (int k = 0; k < SKIP_NCNT; ++k) part[k] += counts[b * SKIP_NCNT + k];
    }
#pragma unroll
    for (int k = 0; k < SKIP_NCNT; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part[k] += __shfl_xor(part[k], d);
        if (lane == 0 && part[k]) atomicAdd(&s_base[k], part[k]);
    }
    const SkipXItem it = skipx_item(i, n, bands, cols, words[SK_EMPTY_RANGE] != 0, bgrows != 0);
    // inclusive scans over the workgroup: inside the wave by shuffles, the waves' totals through LDS
    uint32_t sc[2] = {it.full ? 1u : 0u, (uint32_t)it.wpasses};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(sc[k], d); if (lane >= d) sc[k] += v; }
        if (lane == 63) s_wave[k][wave] = sc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += s_wave[k][w];
        sc[k] += before;
    }
    if (it.full) list[s_base[0] + sc[0] - 1] = i;
    if (it.wpasses) {
        const uint32_t at = s_base[2] + sc[1] - (uint32_t)it.wpasses;
        for (int k = 0; k < it.wpasses; ++k) { wlist[at + k] = skipx_pack(skipx_pass(i, it.rows, it.t0, k)); wrows[at + k] = skipx_v2_pack(it.v2); }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == SKIP_LB - 1) {               // the last block knows the lengths
        const uint32_t full = s_base[0] + sc[0], wp = s_base[2] + sc[1];
        uint32_t need = s_base[1], wc = s_base[3];
        for (int k = 0; k < 2; ++k) { const uint32_t c = counts[blockIdx.x * SKIP_NCNT + 1 + 2 * k]; if (k) wc += c; else need += c; }
        for (int k = 0; k < SKIP_PAD; ++k) list[full + k] = n_pass;
        // SK_LEN, SK_NPASS, SK_FILLED: the aligned passes the row rule lists and the rows outside them (the batch's last pass may be short), whoever
        // supplies those rows
        const bool last_need = skip_needed(n_pass - 1, total_pairs, bands, words[SK_EMPTY_RANGE] != 0);
        const uint32_t listed_rows = need * SkipGeom::RPP - (last_need ? (uint32_t)(n_pass * SkipGeom::RPP - total_pairs) : 0u);
        words[SK_LEN] = need; words[SK_NPASS] = (uint32_t)n_pass; words[SK_FILLED] = (uint32_t)total_pairs - listed_rows;
        if (cols) {                                                        // (null: nobody reads the windowed list or its words)
            for (int k = 0; k < SKIP_PAD; ++k) { wlist[wp + k] = 0; wrows[wp + k] = skipx_v2_pack(SKIPX_V2_ALL); }
            words[SKX_CROPS] = wc; words[SKX_PASSES] = wp; words[SKX_FULL] = full; words[SKX_CTR] = 0;
            words[SKX_V2_READ] = s_base[4] + counts[blockIdx.x * SKIP_NCNT + 4]; words[SKX_V2_MADE] = s_base[5] + counts[blockIdx.x * SKIP_NCNT + 5];
        }
    }
}
// V3 row r of crop c is computed where c has a window and needs the row, or where its aligned pass is on the full-width list; every other row
// <- the empty crop's.  (No crop with a window: the rows of the passes the row rule does not list.)  A thread looks at one of the block's
// SKIP_FILL_TB consecutive V3 rows, then the block copies the rows that are not computed; nothing to copy where the listed conv3 reads the
// image itself
__global__ __launch_bounds__(SKIP_FILL_TB) void k_v3_fill(const int2* __restrict__ bands, const int2* __restrict__ cols, const int n, const uint32_t* __restrict__ words,
                                                          const uint4* __restrict__ v3e, uint4* __restrict__ v3, const int direct) {
    using G = SkipGeom;
    constexpr int ROWQ = V3_ROWB / 16;
    __shared__ unsigned long long s_fill[SKIP_FILL_TB / 64];
    if (direct && words[SK3_USE]) return;
    const bool all = words[SK_EMPTY_RANGE] != 0;
    const int total_pairs = n * G::V3_ROWS, tid = threadIdx.x, gp0 = blockIdx.x * SKIP_FILL_TB;
    {
        const int gp = gp0 + tid;
        bool fill = false;
        if (gp < total_pairs && !all) {
            const int crop = gp / G::V3_ROWS, r = gp - crop * G::V3_ROWS;
            if (!cols) fill = !skip_pass_needed(gp / G::RPP, total_pairs, SkipBandsOf{bands});      // (uniform across the grid)
            else {
                const SkipXWinOf win{cols, all};
                bool computed = false;
                if (win(crop) >= 0) { const int2 b = bands[crop]; const SkipRows need = skip_rows({b.x, b.y}); computed = r >= need.lo && r <= need.hi; }
                fill = !computed && !skipx_full_needed(gp / G::RPP, total_pairs, SkipBandsOf{bands}, win);
            }
        }
        const unsigned long long m = __ballot(fill);
        if ((tid & 63) == 0) s_fill[tid >> 6] = m;
    }
    __syncthreads();
    for (int w = 0; w < SKIP_FILL_TB / 64; ++w) {
        unsigned long long m = s_fill[w];
        while (m) {
            const int gp = gp0 + w * 64 + __ffsll((long long)m) - 1;
            m &= m - 1;
            for (int q = tid; q < ROWQ; q += SKIP_FILL_TB) v3[(size_t)gp * ROWQ + q] = v3e[(gp % G::V3_ROWS) * ROWQ + q];
        }
    }
}

// ---- the listed form of conv3 ----
static constexpr int SKIP3_TB = 256;      // threads per workgroup of the count / list kernels: SKIP3_TB * Skip3Geom::BLOCK crops

// the listed pairs of the workgroup's SKIP3_TB * BLOCK crops into LDS, one byte each for the first pair and the count, crop k of thread t at
// [k][t]: read with coalesced loads here, walked by one thread per BLOCK crops from LDS in a loop that stays small (a walk unrolled over
// registers is 30 KB of code that every thread runs once, from a cold instruction cache: 35 us for what is 800 threads' work)
// (cols not null: the crops whose blob fits a window of WT3 conv3 tiles carry t0 + 1 in bits 12 ..: their runs go into the windowed list)
// The count / list kernels run SKIP3_NT = 2 SKIP3_TB threads: the first SKIP3_TB walk the full-width list of their BLOCK crops, the others -- whole
// waves -- the windowed list of the same crops at the same time (one thread walking both lists, in one loop or in two, was 1.6 times the time of
// these kernels, which is that loop's latency)
// (TILED: four groups -- the lists of tile slots that the kernel walks, and behind them the two lists of pair slots, which are only counted)
static constexpr int SKIP3_NT = 2 * SKIP3_TB, SKIP3_NT_TILED = 4 * SKIP3_TB;
template <int NT>
__device__ __forceinline__ void skip3_stage_runs(const int2* __restrict__ bands, const int2* __restrict__ cols, const int n, const bool all, uint16_t* s_run) {
    using G = Skip3Geom;
    const int c0 = blockIdx.x * SKIP3_TB * G::BLOCK;
    constexpr int U = 8;              // loads in flight per thread: one after the other they are BLOCK round trips to memory
    static_assert(G::BLOCK % U == 0 && (SKIP3_TB * G::BLOCK) % (U * NT) == 0, "whole groups of loads");
    for (int i0 = threadIdx.x; i0 < SKIP3_TB * G::BLOCK; i0 += U * NT) {
        int2 b[U], c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * NT;
            b[u] = c0 + i < n ? bands[c0 + i] : make_int2(SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1);
            c[u] = cols && c0 + i < n ? cols[c0 + i] : make_int2(SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * NT;
            const SkipPairs r = all && c0 + i < n ? SkipPairs{0, G::PAIRS - 1} : skip3_pairs({b[u].x, b[u].y});
            const int t0 = skip3_window({c[u].x, c[u].y}, all);
            s_run[(i % G::BLOCK) * SKIP3_TB + i / G::BLOCK] = (uint16_t)(r.lo <= r.hi ? r.lo | (r.hi - r.lo + 1) << 8 | (t0 + 1) << 12 : 0);
        }
    }
    __syncthreads();
}
// the row pairs of the crops of block `blk` (column t of s_run) that belong to list G -- Skip3XGeom: the crops with a window, Skip3Geom: the others --
// packed into passes (numbered from `passes` on); emit(index, pass) takes each; crops: how many took part; -> pairs listed
template <class G, class E>
__device__ __forceinline__ int skip3_walk(const uint16_t* s_run, const int t, const int blk, int& passes, int& crops, E&& emit) {
    constexpr bool WIN = G::TILES != Skip3Geom::TILES, TILED = Skip3Tiled<G>::value;
    std::conditional_t<TILED, Skip3TPass, Skip3Pass> p{};
    int listed = 0;
#pragma unroll 1
    for (int k = 0; k < G::BLOCK; ++k) {
        const int r = s_run[k * SKIP3_TB + t], len = (r >> 8) & 0xf;
        if (len && ((r >> 12) != 0) == WIN) {
            listed += len;
            ++crops;
            const int gp = (blk * G::BLOCK + k) * G::PAIRS + (r & 0xff);
            if constexpr (TILED) skip3t_add_run<G>(p, passes, gp, len, emit);
            else skip3_add_run<G>(p, passes, gp, len, emit);
        }
    }
    if constexpr (TILED) skip3t_flush(p, passes, emit);
    else skip3_flush(p, passes, emit);
    return listed;
}

// (cols null: no crop has a window, one list, as before there were windows; the second half of the workgroup has nothing to walk)
// (counts: [0 .. grid) of the lists the kernel walks; [grid .. 2 grid) the passes of pair slots, full-width and windowed -- the same numbers
// where the kernel walks those)
template <bool TILED>
__global__ __launch_bounds__(TILED ? SKIP3_NT_TILED : SKIP3_NT) void k_pair_count(const int2* __restrict__ bands, const int2* __restrict__ cols, const int n, const uint32_t* __restrict__ words,
                                                         uint4* __restrict__ counts /* per workgroup: full-width passes, pairs, windowed passes, windowed crops */,
                                                         uint32_t* __restrict__ tcounts /* per block of crops: full-width passes, windowed passes */) {
    __shared__ uint32_t s_pass, s_pair, s_wpass, s_wcrop, s_ppass, s_pwpass;
    __shared__ uint16_t s_run[SKIP3_TB * Skip3Geom::BLOCK];
    if (threadIdx.x == 0) { s_pass = 0; s_pair = 0; s_wpass = 0; s_wcrop = 0; s_ppass = 0; s_pwpass = 0; }
    skip3_stage_runs<TILED ? SKIP3_NT_TILED : SKIP3_NT>(bands, cols, n, words[SK_EMPTY_RANGE] != 0, s_run);
    const int grp = threadIdx.x / SKIP3_TB;                   // (whole waves)
    const bool win = grp & 1;
    const int t = threadIdx.x & (SKIP3_TB - 1), blk = blockIdx.x * SKIP3_TB + t;
    if (blk * Skip3Geom::BLOCK < n) {
        int passes = 0, crops = 0, listed = 0;
        const auto none = [](int, const auto&) {};
        if (grp >= 2) {                                       // TILED only: the passes of pair slots, counted
            if (!win) skip3_walk<Skip3Geom>(s_run, t, blk, passes, crops, none);
            else if (cols) skip3_walk<Skip3XGeom>(s_run, t, blk, passes, crops, none);
            if (passes) atomicAdd(win ? &s_pwpass : &s_ppass, (uint32_t)passes);
        } else {
            if (!win) listed = skip3_walk<std::conditional_t<TILED, Skip3TGeom, Skip3Geom>>(s_run, t, blk, passes, crops, none);
            else if (cols) listed = skip3_walk<std::conditional_t<TILED, Skip3TXGeom, Skip3XGeom>>(s_run, t, blk, passes, crops, none);
            tcounts[2 * blk + (win ? 1 : 0)] = (uint32_t)passes;
            if (passes) atomicAdd(win ? &s_wpass : &s_pass, (uint32_t)passes);
            if (listed) atomicAdd(&s_pair, (uint32_t)listed);
            if (win && crops) atomicAdd(&s_wcrop, (uint32_t)crops);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = make_uint4(s_pass, s_pair, s_wpass, s_wcrop);
        counts[gridDim.x + blockIdx.x] = TILED ? make_uint4(s_ppass, s_pwpass, 0, 0) : make_uint4(s_pass, s_wpass, 0, 0);
    }
}

template <bool TILED>
__global__ __launch_bounds__(SKIP3_NT) void k_pair_list(const int2* __restrict__ bands, const int2* __restrict__ cols, const int n, uint32_t* __restrict__ words,
                                                        const uint4* __restrict__ counts, const uint32_t* __restrict__ tcounts, int* __restrict__ desc,
                                                        int* __restrict__ xdesc /* the windowed passes, Skip3XGeom::DESC words each, either form */) {
    using G = std::conditional_t<TILED, Skip3TGeom, Skip3Geom>;
    using X = std::conditional_t<TILED, Skip3TXGeom, Skip3XGeom>;
    __shared__ uint2 s_scan[SKIP3_TB];
    __shared__ uint16_t s_run[SKIP3_TB * G::BLOCK];
    const int tid = threadIdx.x, t = tid & (SKIP3_TB - 1), blk = blockIdx.x * SKIP3_TB + t;
    const bool win = tid >= SKIP3_TB;                         // (whole waves)
    const bool mine = blk * G::BLOCK < n;
    skip3_stage_runs<SKIP3_NT>(bands, cols, n, words[SK_EMPTY_RANGE] != 0, s_run);
    // the passes in front of this workgroup (all of them, and the pairs: the last workgroup writes the counters)
    uint32_t before = 0, wbefore = 0, pairs = 0, wcrops = 0, ppasses = 0, pwpasses = 0;
    for (int b = 0; b <= (int)blockIdx.x; ++b) {
        const uint4 c = counts[b], pc = counts[gridDim.x + b];
        if (b < (int)blockIdx.x) { before += c.x; wbefore += c.z; }
        pairs += c.y; wcrops += c.w; ppasses += pc.x; pwpasses += pc.y;
    }
    const uint2 cnt = mine ? make_uint2(tcounts[2 * blk], tcounts[2 * blk + 1]) : make_uint2(0, 0);
    if (!win) s_scan[t] = cnt;
    __syncthreads();
    for (int d = 1; d < SKIP3_TB; d <<= 1) {          // inclusive scan, by the first half
        const uint2 v = !win && t >= d ? s_scan[t - d] : make_uint2(0, 0);
        __syncthreads();
        if (!win) { s_scan[t].x += v.x; s_scan[t].y += v.y; }
        __syncthreads();
    }
    int at = win ? (int)(wbefore + s_scan[t].y - cnt.y) : (int)(before + s_scan[t].x - cnt.x), crops = 0;
    // (the pass as its runs, in the first words of its descriptor: k_act3_fill makes the descriptor of it, a thread per pass; TILED: o and the
    // tile count beside run A's pairs, as in word S3_TILES, 8 bits further up)
    const auto runs_of = [](const auto& p) {
        int la = p.len[0];
        if constexpr (std::is_same_v<std::decay_t<decltype(p)>, Skip3TPass>) la |= (p.o | p.n << S3_COUNT_SHIFT) << 8;
        return make_int4(p.gp0[0], la, p.gp0[1], p.runs > 1 ? p.len[1] : 0);
    };
    if (mine && !win)
        skip3_walk<G>(s_run, t, blk, at, crops, [&](const int idx, const auto& p) { *reinterpret_cast<int4*>(desc + (size_t)idx * G::DESC) = runs_of(p); });
    if (mine && win && cols)
        skip3_walk<X>(s_run, t, blk, at, crops, [&](const int idx, const auto& p) { *reinterpret_cast<int4*>(xdesc + (size_t)idx * X::DESC) = runs_of(p); });
    if (blockIdx.x == gridDim.x - 1 && tid == SKIP3_TB - 1) {
        const uint32_t listed = before + s_scan[t].x, wlisted = wbefore + s_scan[t].y;
        const long long dense = ((long long)n * (G::PAIRS * 10) + 63) / 64;      // the dense form's passes: 64 of the crop's 100 tiles each
        // (the counters and the choice stay those of the passes of pair slots, whichever lists the kernel walks: SK3_RAN, SK3X_RAN)
        words[SK3_PAIRS] = (uint32_t)(n * G::PAIRS); words[SK3_LISTED] = pairs; words[SK3_PASSES] = ppasses; words[SK3_FILLED] = 0;
        words[SK3X_PASSES] = pwpasses; words[SK3X_CROPS] = wcrops; words[SK3X_CTR] = 0;
        words[SK3_RAN] = listed; words[SK3X_RAN] = wlisted;
        // (a windowed pass is counted as a full-width one: 117.6 against 116.2 ns under a kernel trace, profiles/conv3_windowed.txt)
        words[SK3_USE] = skip3_use_list((long long)ppasses + pwpasses, dense) ? 1u : 0u;
    }
}

// ---- the listed form of fc1 ----
// Plane q's list: the crops whose pair q is listed (skip3_fc1_listed), ascending, at list[q * stride ..], and its length in words[SK3_FC1_LEN + q].
// One workgroup per plane, no atomics, nothing between workgroups: a wave looks at 64 consecutive crops at a time (one ballot = one 64-bit word of
// the plane's bit map in LDS), a thread per word counts, one scan over the workgroup gives every word its place, and the waves write their words'
// crops out, coalesced.  FC1L_SEG crops per round; every batch the role-split chain has seen is one round.
static constexpr int FC1L_TB = 1024, FC1L_SEG = FC1L_TB * 64;
__global__ __launch_bounds__(FC1L_TB) void k_fc1_list(const int2* __restrict__ bands, const int n, uint32_t* __restrict__ words,
                                                      int* __restrict__ list /*[PAIRS][stride]*/, const int stride) {
    constexpr int NW = FC1L_TB / 64, U = 8;
    __shared__ unsigned long long s_mask[FC1L_TB];
    __shared__ uint32_t s_off[FC1L_TB], s_wave[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
    const bool all = words[SK_EMPTY_RANGE] != 0;
    int* out = list + (size_t)q * stride;
    uint32_t base = 0;
    for (int seg0 = 0; seg0 < n; seg0 += FC1L_SEG) {
        const int left = n - seg0, nw = left >= FC1L_SEG ? FC1L_TB : (left + 63) / 64;      // bit-map words of this round
        for (int w0 = wave; w0 < nw; w0 += U * NW) {          // U loads in flight per lane
            int2 b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int crop = seg0 + (w0 + u * NW) * 64 + lane;
                b[u] = w0 + u * NW < nw && crop < n ? bands[crop] : make_int2(SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int crop = seg0 + (w0 + u * NW) * 64 + lane;
                const unsigned long long m = __ballot(crop < n && skip3_fc1_listed(all, {b[u].x, b[u].y}, q));
                if (lane == 0 && w0 + u * NW < nw) s_mask[w0 + u * NW] = m;
            }
        }
        __syncthreads();
        const uint32_t cnt = tid < nw ? (uint32_t)__popcll(s_mask[tid]) : 0u;
        uint32_t incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d); if (lane >= d) incl += v; }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = base, total = base;
        for (int w = 0; w < NW; ++w) { const uint32_t c = s_wave[w]; if (w < wave) before += c; total += c; }
        s_off[tid] = before + incl - cnt;
        __syncthreads();
        for (int w = wave; w < nw; w += NW) {
            const unsigned long long m = s_mask[w];
            if ((m >> lane) & 1ull) out[s_off[w] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = seg0 + w * 64 + lane;
        }
        base = total;
        __syncthreads();
    }
    if (tid == 0) words[SK3_FC1_LEN + q] = base;
}

// a thread per listed pass: its descriptor; then SKIP3_FC crops per workgroup, a wave after the other: the row pairs outside the listed range
// <- the empty crop's (a pair is 10 x 128 floats).  Nothing to do when the dense form runs.  (n * 16 threads, fewer than 3 n passes.)  One add to
// the counter per workgroup: an add per crop is 25600 of them on one word, and they took longer than the copy
static constexpr int SKIP3_FC = 16;
// cols (null: no crop has a window): the windowed passes' descriptors and row sources as well (xdesc, xrows), and of every LISTED pair of a crop
// with a window the pooled columns outside it <- the empty crop's: the windowed kernel does not write them, and fc1 -- listed or not -- reads
// whole pairs.  These are not counted: SK3_FILLED is the row rule's
template <bool TILED>
__global__ __launch_bounds__(256) void k_act3_fill(const int2* __restrict__ bands, const int2* __restrict__ cols, const int n, uint32_t* __restrict__ words,
                                                   const uint4* __restrict__ act3e, uint4* __restrict__ act3, int* __restrict__ desc,
                                                   uint32_t* __restrict__ rows /* Skip3Reach::WORDS per pass */,
                                                   int* __restrict__ xdesc, uint32_t* __restrict__ xrows /* TILED: Skip3TXGeom::ROW_WORDS per pass */,
                                                   const long long alloc_rows /* V3 rows in front of the back image */, const int direct,
                                                   const int copy /* 0: the listed fc1 runs and reads no unlisted pair -- they are counted, not copied */) {
    using G = std::conditional_t<TILED, Skip3TGeom, Skip3Geom>;
    constexpr int PQ = 10 * 128 * 4 / 16;             // 16-byte units per pair
    using X = std::conditional_t<TILED, Skip3TXGeom, Skip3XGeom>;
    constexpr int CQ = 128 * 4 / 16;                  // 16-byte units per pooled column of a pair
    static_assert((G::BLOCK_PASSES + X::BLOCK_PASSES) * SKIP3_FC <= Skip3Geom::BLOCK * 256 && SKIP3_FC % 4 == 0, "a thread per pass of either list: 256 threads per SKIP3_FC crops");
    // the runs k_pair_list left -> the pass as its pairs, and o | tiles << 8 (TILED)
    const auto pass_of = [](const int4 r, int& tiles) {
        Skip3Pass p{};
        const int la = TILED ? r.y & 0xff : r.y;
        tiles = TILED ? r.y >> 8 : 0;
        p.runs = r.w ? 2 : 1; p.n = la + r.w;
        p.gp0[0] = r.x; p.len[0] = la; p.gp0[1] = r.z; p.len[1] = r.w;
        return p;
    };
    __shared__ uint32_t s_filled;
    const int lane = threadIdx.x & 63;
    if (!words[SK3_USE]) return;
    if (threadIdx.x == 0) s_filled = 0;
    __syncthreads();
    const bool all = words[SK_EMPTY_RANGE] != 0;
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int n_full = (int)words[SK3_RAN], n_win = cols ? (int)words[SK3X_RAN] : 0;
    const SkipRows every{0, SkipGeom::V3_ROWS - 1};
    const bool from_v3 = all || !direct;
    if (gid >= n_full && gid - n_full < n_win) {          // a windowed pass: the same, with its crops' windows
        int4* dst = reinterpret_cast<int4*>(xdesc + (size_t)(gid - n_full) * X::DESC);
        const int4 r = dst[0];
        int tiles;
        const Skip3Pass p = pass_of(r, tiles);
        const int ca = r.x / X::PAIRS, cb = (r.w ? r.z : r.x) / X::PAIRS;
        const int2 xa = cols[ca], xb = cols[cb];
        const int t0a = skip3_window({xa.x, xa.y}, all), t0b = skip3_window({xb.x, xb.y}, all);
        int d[X::DESC];
        skip3_describe<X>(p, d, t0a, t0b);
        if (TILED) d[S3_TILES] = tiles;
#pragma unroll
        for (int k = 0; k < X::DESC / 4; ++k) dst[k] = make_int4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
        const int2 ba = bands[ca], bb = bands[cb];
        // (TILED: a windowed pass can stage 32 rows, and its row table is one of 64 words)
        constexpr int XW = TILED ? Skip3TXGeom::ROW_WORDS : Skip3Reach::WORDS;
        unsigned w[XW];
        const SkipRows oa = from_v3 ? every : skip_rows({ba.x, ba.y}), ob = from_v3 ? every : skip_rows({bb.x, bb.y});
        if constexpr (TILED) skip3t_row_words<X>(p, oa, ob, alloc_rows, w, t0a, t0b);
        else skip3_row_words<X>(p, oa, ob, alloc_rows, w, t0a, t0b);
        uint4* wd = reinterpret_cast<uint4*>(xrows + (size_t)(gid - n_full) * XW);
#pragma unroll
        for (int k = 0; k < XW / 4; ++k) wd[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
    if (gid < n_full) {
        int4* dst = reinterpret_cast<int4*>(desc + (size_t)gid * G::DESC);
        const int4 r = dst[0];
        int tiles;
        const Skip3Pass p = pass_of(r, tiles);
        int d[G::DESC];
        skip3_describe<G>(p, d);
        if (TILED) d[S3_TILES] = tiles;
#pragma unroll
        for (int k = 0; k < G::DESC / 4; ++k) dst[k] = make_int4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
        // where its rows come from: the own rows of its crops from V3, the others from the image -- or all of them from V3, where the copy is kept
        const int2 ba = bands[r.x / G::PAIRS], bb = bands[(r.w ? r.z : r.x) / G::PAIRS];
        unsigned w[Skip3Reach::WORDS];
        skip3_row_words<G>(p, from_v3 ? every : skip_rows({ba.x, ba.y}), from_v3 ? every : skip_rows({bb.x, bb.y}), alloc_rows, w);
        uint4* wd = reinterpret_cast<uint4*>(rows + (size_t)gid * Skip3Reach::WORDS);
#pragma unroll
        for (int k = 0; k < Skip3Reach::WORDS / 4; ++k) wd[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
    uint32_t filled = 0;
    for (int k = 0; k < SKIP3_FC / 4; ++k) {
        const int crop = blockIdx.x * SKIP3_FC + (threadIdx.x >> 6) * (SKIP3_FC / 4) + k;
        if (crop >= n) break;
        const int2 b = bands[crop];
        const SkipPairs r = all ? SkipPairs{0, G::PAIRS - 1} : skip3_pairs({b.x, b.y});
        const int2 c = cols ? cols[crop] : make_int2(SKIP_BAND_NONE.y0, SKIP_BAND_NONE.y1);
        const int t0 = skip3_window({c.x, c.y}, all);
        for (int q = 0; q < G::PAIRS; ++q) {
            if (q >= r.lo && q <= r.hi) {
                if (t0 >= 0) {        // the pooled columns in front of the window's 2 WT3 and behind them
                    constexpr int OUT = (10 - 2 * X::WT3) * CQ;
                    for (int i = lane; i < OUT; i += 64) {
                        const int u = i < 2 * t0 * CQ ? i : i + 2 * X::WT3 * CQ;
                        act3[((size_t)crop * G::PAIRS + q) * PQ + u] = act3e[q * PQ + u];
                    }
                }
                continue;
            }
            ++filled;
            if (!copy) continue;
#pragma unroll
            for (int i = lane; i < PQ; i += 64) act3[((size_t)crop * G::PAIRS + q) * PQ + i] = act3e[q * PQ + i];
        }
    }
    if (lane == 0 && filled) atomicAdd(&s_filled, filled);
    __syncthreads();
    if (threadIdx.x == 0 && s_filled) atomicAdd(&words[SK3_FILLED], s_filled);
}
