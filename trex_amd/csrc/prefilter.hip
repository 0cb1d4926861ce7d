// prefilter.hip -- Tracker::prefilter's blob policy on the device (tracking/Tracker.cpp:742-914, PrefilterBlobs.cpp:130-150, :328-385,
// core/SizeFilters.cpp): behind the re-threshold pass (segment.hip, launch_rethreshold) every detect blob and every sub-blob is sorted into
// committed / big / filtered out (with a reason), the committed and big lists are written in the order the reference's loop appends them,
// and presumed_nr for trexhip_split_search_device is derived from the big list.  Two kernels:
//   k_pre_count2   one wave per counted entry: pixels whose difference is >= track_threshold_2 (Tracker.cpp:866)
//   k_pre_decide   one workgroup per frame: per-parent recount (integer LDS atomics), the checks in the reference's float types, and a
//                  stable compaction (ballot + prefix over the workgroup) of the two lists
// Built with -ffp-contract=off: every product and comparison is the formula's.
#include "internal.h"

namespace trexhip {
namespace {

constexpr int PRE_THREADS = 256;
constexpr int PRE_MAX_SHAPES = 64, PRE_MAX_POINTS = 4096;
constexpr size_t PRE_LDS_LIMIT = 160 * 1024;
constexpr int32_t PRE_NOT_COUNTED = -1, PRE_WANTED = -2;

struct PreCfg {
    int W, H, B, invert, method, thr, thr2;
    int n_ranges;
    float sqcm, ratio_lo, ratio_hi;
    double ranges[16];
    double min_start, max_end;          // SizeFilters::max_range() (SizeFilters.cpp:12-18)
    int n_inc, n_inc_pts, n_ign, n_ign_pts, n_bdx;
    uint32_t cap;                       // pooled blob capacity = max_batch * max_blobs: entries >= cap are detect blobs
    uint32_t per_frame;                 // entries of d_order / the sequence scratch per frame = 2 * max_blobs
    uint32_t mb;                        // max_blobs: sub-blob k of frame f is entry f * mb + k, its detect blob k entry cap + f * mb + k
    uint32_t n1max;                     // most detect blobs of a frame of this batch (sizes the per-parent LDS arrays)
};

__device__ __forceinline__ int pre_diff(int p, int b, int method) { return method == 0 ? abs(b - p) : (method == 1 ? max(b - p, 0) : p); }

// SizeFilters::in_range_of_one(cmsq) (SizeFilters.cpp:36-53, scale_factor -1): Range<double>::contains = [start, end)
__device__ __forceinline__ bool pre_in_range(float cmsq, const PreCfg& c) {
    if (c.n_ranges <= 0) return true;
    const double v = (double)cmsq;
    for (int i = 0; i < c.n_ranges; ++i)
        if (v >= c.ranges[2 * i] && v < c.ranges[2 * i + 1]) return true;
    return false;
}
// SizeFilters::close_to_minimum_of_one(cmsq, 0.5) (SizeFilters.cpp:20-26)
__device__ __forceinline__ bool pre_close_to_minimum(float cmsq, const PreCfg& c) {
    for (int i = 0; i < c.n_ranges; ++i)
        if ((double)cmsq >= c.ranges[2 * i] * (double)0.5f) return true;
    return false;
}

struct Shapes { const float2* pts; const int* off; int n, n_pts; };

__device__ __forceinline__ void shape_span(const Shapes& s, int k, int& a, int& b) {
    a = min(max(s.off[k], 0), s.n_pts);
    b = min(max(s.off[k + 1], a), s.n_pts);
}

// PrefilterBlobs::blob_matches_shapes (PrefilterBlobs.cpp:328-355) on the blob's centre
__device__ bool pre_matches(const Shapes& s, float cx, float cy) {
    for (int k = 0; k < s.n; ++k) {
        int a, b;
        shape_span(s, k, a, b);
        const int n = b - a;
        if (n == 2) {                                                     // Bounds(rect[0], rect[1] - rect[0]).contains(center)
            const float x = s.pts[a].x, y = s.pts[a].y, w = s.pts[a + 1].x - x, h = s.pts[a + 1].y - y;
            if (cx >= x && cx < x + w && cy >= y && cy < y + h) return true;
        } else if (n > 2) {                                               // pnpoly: W. R. Franklin's crossing test
            bool in = false;
            for (int i = 0, j = n - 1; i < n; j = i++) {
                const float xi = s.pts[a + i].x, yi = s.pts[a + i].y, xj = s.pts[a + j].x, yj = s.pts[a + j].y;
                if (((yi > cy) != (yj > cy)) && (cx < (xj - xi) * (cy - yi) / (yj - yi) + xi)) in = !in;
            }
            if (in) return true;
        }
    }
    return false;
}

// PrefilterBlobs::rect_overlaps_shapes (PrefilterBlobs.cpp:357-385) on the blob's bounds
__device__ bool pre_overlaps(const Shapes& s, float bx, float by, float bw, float bh) {
    for (int k = 0; k < s.n; ++k) {
        int a, b;
        shape_span(s, k, a, b);
        const int n = b - a;
        float x, y, w, h;
        if (n == 2) {
            x = s.pts[a].x; y = s.pts[a].y; w = s.pts[a + 1].x - x; h = s.pts[a + 1].y - y;
        } else if (n > 2) {                                               // :364-369, as written: the box starts as (0, 0, FLT_MAX, FLT_MAX)
            x = 0.f; y = 0.f; w = 3.402823466e+38f; h = 3.402823466e+38f;
            for (int i = a; i < b; ++i) {                                 // Bounds::insert_point: x, y = minimum, width, height = maximum
                x = fminf(x, s.pts[i].x); y = fminf(y, s.pts[i].y);
                w = fmaxf(w, s.pts[i].x); h = fmaxf(h, s.pts[i].y);
            }
            w -= x; h -= y;
        } else continue;
        if (x < bx + bw && bx < x + w && y < by + bh && by < y + h) return true;   // Bounds::overlaps
    }
    return false;
}

// std::set<pv::bid>::contains on the frame's sorted list
__device__ __forceinline__ bool pre_bdx_contains(const uint32_t* list, int lo, int hi, uint32_t bid) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t v = list[mid];
        if (v == bid) return true;
        if (v < bid) lo = mid + 1; else hi = mid;
    }
    return false;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// pixels [0, n) of one line, all 64 lanes: 16-byte loads where both rows allow them
__device__ int count_long_run(const uint8_t* img, const uint8_t* bgp, int n, int lane, const PreCfg& c) {
    int cnt = 0;
    if ((((uintptr_t)img ^ (uintptr_t)bgp) & 15) != 0) {
        for (int i = lane; i < n; i += 64) { int p = img[i]; if (c.invert) p = 255 - p; cnt += pre_diff(p, bgp[i], c.method) >= c.thr2; }
        return cnt;
    }
    const int head = min(n, (int)((16 - ((uintptr_t)img & 15)) & 15));
    if (lane < head) { int p = img[lane]; if (c.invert) p = 255 - p; cnt += pre_diff(p, bgp[lane], c.method) >= c.thr2; }
    const int nb = (n - head) >> 4;
    for (int k = lane; k < nb; k += 64) {
        const uint4 a = *reinterpret_cast<const uint4*>(img + head + 16 * k);
        const uint4 b = *reinterpret_cast<const uint4*>(bgp + head + 16 * k);
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int p = (int)((aw[w] >> (8 * q)) & 255u);
                if (c.invert) p = 255 - p;
                cnt += pre_diff(p, (int)((bw[w] >> (8 * q)) & 255u), c.method) >= c.thr2;
            }
    }
    for (int i = head + 16 * nb + lane; i < n; i += 64) { int p = img[i]; if (c.invert) p = 255 - p; cnt += pre_diff(p, bgp[i], c.method) >= c.thr2; }
    return cnt;
}

// One wave per blob whose entry the gate pass marked PRE_WANTED: e < tot2 = pooled sub-blob e, else pooled detect blob e - tot2.  Lines
// shorter than 32 pixels are counted one per lane; longer ones by the whole wave with 16-byte loads.
__global__ __launch_bounds__(PRE_THREADS) void k_pre_count2(const PreCfg c, const uint8_t* __restrict__ frames, const uint8_t* __restrict__ bg,
                                                            const trexhip_frame_info* __restrict__ info1, const uint32_t* __restrict__ bf1,
                                                            const trexhip_blob* __restrict__ blobs1, const trexhip_run* __restrict__ runs1,
                                                            const uint32_t* __restrict__ tot1p,
                                                            const trexhip_frame_info* __restrict__ info2, const uint32_t* __restrict__ bf2,
                                                            const trexhip_blob* __restrict__ blobs2, const trexhip_run* __restrict__ runs2,
                                                            const uint32_t* __restrict__ tot2p, int32_t* __restrict__ count2) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * PRE_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * PRE_THREADS) >> 6;
    const uint32_t tot1 = min(tot1p[0], c.cap), tot2 = min(tot2p[0], c.cap);
    for (uint32_t e = wave; e < tot1 + tot2; e += n_waves) {
        const bool sub = e < tot2;
        const uint32_t bi = sub ? e : e - tot2;
        const uint32_t f = sub ? bf2[bi] : bf1[bi];
        if (f >= (uint32_t)c.B) continue;
        const trexhip_frame_info fi = sub ? info2[f] : info1[f];
        const uint32_t k = bi - fi.blob_begin;                            // index in the frame
        if (fi.flags || k >= c.mb || k >= fi.n_blobs) continue;
        int32_t* out = count2 + (sub ? 0u : c.cap) + f * c.mb + k;
        if (*out != PRE_WANTED) continue;                                 // wave-uniform
        const trexhip_blob B = sub ? blobs2[bi] : blobs1[bi];
        const trexhip_run* rr = (sub ? runs2 : runs1) + fi.run_begin + B.run_begin;
        const uint8_t* img = frames + (size_t)f * c.H * c.W;
        int cnt = 0;
        for (uint32_t r0 = 0; r0 < B.n_runs; r0 += 64) {
            const uint32_t r = r0 + lane;
            trexhip_run q = {};
            bool ok = false;
            if (r < B.n_runs) { q = rr[r]; ok = q.y < c.H && q.x1 < c.W && q.x0 <= q.x1; }
            const int len = ok ? q.x1 - q.x0 + 1 : 0;
            if (len > 0 && len < 32) {
                const uint8_t* ip = img + (size_t)q.y * c.W + q.x0;
                const uint8_t* bp = bg + (size_t)q.y * c.W + q.x0;
                for (int i = 0; i < len; ++i) { int p = ip[i]; if (c.invert) p = 255 - p; cnt += pre_diff(p, bp[i], c.method) >= c.thr2; }
            }
            unsigned long long longs = __ballot(len >= 32);
            while (longs) {
                const int src = __ffsll((long long)longs) - 1;
                longs &= longs - 1;
                const int y = __shfl((int)q.y, src, 64), x0 = __shfl((int)q.x0, src, 64), n = __shfl(len, src, 64);
                cnt += count_long_run(img + (size_t)y * c.W + x0, bg + (size_t)y * c.W + x0, n, lane, c);
            }
        }
        cnt = wave_sum(cnt);
        if (lane == 0) *out = cnt;
    }
}

// exclusive prefix of a flag over the workgroup, in thread order: ballot + popcount inside a wave, the four wave totals through LDS
__device__ __forceinline__ uint32_t block_flag_scan(bool flag, uint32_t* s_w, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < PRE_THREADS / 64; ++w) { const uint32_t t = s_w[w]; if (w < wave) off += t; total += t; }
    return off + before;
}

// exclusive prefix of a value over the workgroup, in thread order
__device__ __forceinline__ uint32_t block_value_scan(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += t; }
    __syncthreads();
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t off = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < PRE_THREADS / 64; ++w) { const uint32_t t = s_w[w]; if (w < wave) off += t; total += t; }
    return off + incl - v;
}

// One workgroup per frame.  GATE = 1: only the imprecise check and the close_to_minimum gate, to mark the entries whose second count is
// wanted.  GATE = 0: every decision, the two ordered lists, the counts and presumed_nr.
template <int GATE>
__global__ __launch_bounds__(PRE_THREADS) void k_pre_decide(const PreCfg c, const trexhip_frame_info* __restrict__ info1, const trexhip_blob* __restrict__ blobs1,
                                                            const trexhip_frame_info* __restrict__ info2, const trexhip_blob* __restrict__ blobs2,
                                                            const float2* __restrict__ inc_pts, const int* __restrict__ inc_off,
                                                            const float2* __restrict__ ign_pts, const int* __restrict__ ign_off,
                                                            const uint32_t* __restrict__ bdx, const int* __restrict__ bdx_off,
                                                            int32_t* __restrict__ count2, int32_t* __restrict__ seq,
                                                            uint8_t* __restrict__ decision, int32_t* __restrict__ order, int32_t* __restrict__ counts,
                                                            int32_t* __restrict__ presumed) {
    extern __shared__ __align__(16) uint8_t lds_raw[];
    __shared__ uint32_t s_w[PRE_THREADS / 64];
    __shared__ uint32_t s_par[PRE_THREADS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const trexhip_frame_info f1 = info1[f], f2 = info2[f];
    if (f1.flags || f2.flags) {                                           // overflowed / malformed: the frame decides nothing
        if (!GATE && tid < 4) counts[4 * f + tid] = tid == 3 ? 1 : 0;
        return;
    }
    // LDS: shape tables, then three words per detect blob of the frame
    float2* s_pts = reinterpret_cast<float2*>(lds_raw);
    int* s_off = reinterpret_cast<int*>(s_pts + c.n_inc_pts + c.n_ign_pts);
    uint32_t* s_px = reinterpret_cast<uint32_t*>(s_off + (c.n_inc + 1) + (c.n_ign + 1));
    uint32_t* s_cnt = s_px + c.n1max;
    uint32_t* s_state = s_cnt + c.n1max;
    const uint32_t n1 = min(min(f1.n_blobs, c.n1max), c.mb), b1 = f1.blob_begin, n2 = min(f2.n_blobs, c.mb), b2 = f2.blob_begin;
    const uint32_t e2 = (uint32_t)f * c.mb, e1 = c.cap + e2;                 // the frame's first sub-blob entry, first detect-blob entry
    for (int i = tid; i < c.n_inc_pts; i += PRE_THREADS) s_pts[i] = inc_pts[i];
    for (int i = tid; i < c.n_ign_pts; i += PRE_THREADS) s_pts[c.n_inc_pts + i] = ign_pts[i];
    for (int i = tid; i <= c.n_inc; i += PRE_THREADS) s_off[i] = c.n_inc ? inc_off[i] : 0;
    for (int i = tid; i <= c.n_ign; i += PRE_THREADS) s_off[c.n_inc + 1 + i] = c.n_ign ? ign_off[i] : 0;
    for (uint32_t j = tid; j < n1; j += PRE_THREADS) { s_px[j] = 0; s_cnt[j] = 0; }
    __syncthreads();
    const Shapes inc = {s_pts, s_off, c.n_inc, c.n_inc_pts};
    const Shapes ign = {s_pts + c.n_inc_pts, s_off + c.n_inc + 1, c.n_ign, c.n_ign_pts};
    int bl = 0, bh = 0;
    if (bdx) { bl = min(max(bdx_off[f], 0), c.n_bdx); bh = min(max(bdx_off[f + 1], bl), c.n_bdx); }

    // recount of a detect blob = its surviving pixels = the pixels of its sub-blobs (order-free integer sums)
    for (uint32_t i = tid; i < n2; i += PRE_THREADS) {
        const uint32_t p = blobs2[b2 + i].parent - b1;
        if (p < n1) { atomicAdd(&s_px[p], blobs2[b2 + i].n_pixels); atomicAdd(&s_cnt[p], 1u); }
    }
    __syncthreads();

    // per detect blob: check_blob(own, false) (Tracker.cpp:765-801, :816) and the gate of :828-831.
    // state 0 = its sub-blobs are the entries, 1 = the un-thresholded blob is (:853-858), >= 16 = filtered out here
    for (uint32_t j = tid; j < n1; j += PRE_THREADS) {
        const trexhip_blob B = blobs1[b1 + j];
        const float full = (float)B.n_pixels * c.sqcm;
        // :768-774: far beyond the largest range the recount is set without a pixel pass (force_set_recount), else counted
        const float recount = (c.n_ranges > 0 && (double)full > c.max_end * 100.0) ? full : (float)s_px[j] * c.sqcm;
        uint32_t st;
        if (c.n_inc > 0 && !pre_overlaps(inc, (float)B.x0, (float)B.y0, (float)(B.x1 - B.x0 + 1), (float)(B.y1 - B.y0 + 1))) st = 16 + TREXHIP_FILTER_OUTSIDE_INCLUDE;
        else if (pre_bdx_contains(bdx, bl, bh, B.bid)) st = 16 + TREXHIP_FILTER_BDX_IGNORED;
        else {
            const bool gated = (c.n_ranges <= 0 || pre_close_to_minimum(recount, c)) && c.thr > 0;
            st = (gated && s_cnt[j] > 0) ? 0u : 1u;
        }
        s_state[j] = st;
        if (GATE) count2[e1 + j] = (st == 1 && pre_in_range(recount, c)) ? PRE_WANTED : PRE_NOT_COUNTED;
    }
    __syncthreads();
    if (GATE) {
        for (uint32_t i = tid; i < n2; i += PRE_THREADS) {
            const trexhip_blob S = blobs2[b2 + i];
            const uint32_t p = S.parent - b1;
            count2[e2 + i] = (p < n1 && s_state[p] == 0 && pre_in_range((float)S.n_pixels * c.sqcm, c)) ? PRE_WANTED : PRE_NOT_COUNTED;
        }
        return;
    }

    // size test of one entry (Tracker.cpp:861-913)
    auto size_decision = [&](float recount, int32_t second_px) -> uint32_t {
        if (pre_in_range(recount, c)) {
            if (c.thr2 > 0) {
                const float second_count = (float)second_px * c.sqcm;                       // :866
                const float lo = c.ratio_lo * recount, hi = c.ratio_hi * recount;           // :870, Range<float>::contains = [start, end)
                if (!(second_count >= lo && second_count < hi)) return 16 + TREXHIP_FILTER_SECOND_THRESHOLD;
            }
            return 0;
        }
        if (c.n_ranges > 0 && (double)recount < c.min_start) return 16 + TREXHIP_FILTER_OUTSIDE_RANGE;
        return 1;
    };
    // check_precise_not_ignored (:742-763) on the centre of the bounds; parent_bid = 0xFFFFFFFF for a blob without parent
    auto precise = [&](const trexhip_blob& B, bool has_parent, uint32_t parent_bid) -> uint32_t {
        const float cx = (float)B.x0 + (float)(B.x1 - B.x0 + 1) * 0.5f, cy = (float)B.y0 + (float)(B.y1 - B.y0 + 1) * 0.5f;
        if (c.n_ign > 0 && pre_matches(ign, cx, cy)) return 16 + TREXHIP_FILTER_INSIDE_IGNORE;
        if (c.n_inc > 0 && !pre_matches(inc, cx, cy)) return 16 + TREXHIP_FILTER_OUTSIDE_INCLUDE;
        if (pre_bdx_contains(bdx, bl, bh, B.bid) || (has_parent && pre_bdx_contains(bdx, bl, bh, parent_bid))) return 16 + TREXHIP_FILTER_BDX_IGNORED;
        return 0;
    };

    for (uint32_t j = tid; j < n1; j += PRE_THREADS) {
        uint32_t d = s_state[j];
        if (d == 0) d = 255;                                              // its sub-blobs stand for it
        else if (d == 1) {
            const trexhip_blob B = blobs1[b1 + j];
            d = precise(B, false, 0u);
            if (d == 0) {
                const float full = (float)B.n_pixels * c.sqcm;
                const float recount = (c.n_ranges > 0 && (double)full > c.max_end * 100.0) ? full : (float)s_px[j] * c.sqcm;
                d = size_decision(recount, c.thr2 > 0 ? count2[e1 + j] : 0);
            }
        }
        decision[e1 + j] = (uint8_t)d;
    }
    for (uint32_t i = tid; i < n2; i += PRE_THREADS) {
        const trexhip_blob S = blobs2[b2 + i];
        const uint32_t p = S.parent - b1;
        uint32_t d = 255;
        if (p < n1 && s_state[p] == 0) {                                  // check_blob(add, true) (:843)
            d = precise(S, true, blobs1[b1 + p].bid);
            if (d == 0) d = size_decision((float)S.n_pixels * c.sqcm, c.thr2 > 0 ? count2[e2 + i] : 0);
        }
        decision[e2 + i] = (uint8_t)d;
    }
    __syncthreads();

    // the reference's order: detect blob by detect blob, each followed by its sub-blobs in table order.
    // s_cnt -> first slot of the detect blob in the frame's sequence; s_px -> running cursor of its sub-blobs
    uint32_t running = 0;
    for (uint32_t j0 = 0; j0 < n1; j0 += PRE_THREADS) {
        const uint32_t j = j0 + tid;
        const uint32_t v = j < n1 ? 1u + s_cnt[j] : 0u;
        uint32_t total;
        const uint32_t ex = block_value_scan(v, s_w, total);
        if (j < n1) { s_cnt[j] = running + ex; s_px[j] = 0; }
        running += total;
    }
    const uint32_t n_seq = min(running, c.per_frame);
    int32_t* sq = seq + (size_t)f * c.per_frame;
    __syncthreads();
    for (uint32_t j = tid; j < n1; j += PRE_THREADS)
        if (s_cnt[j] < c.per_frame) sq[s_cnt[j]] = (int32_t)(e1 + j);
    for (uint32_t i0 = 0; i0 < n2; i0 += PRE_THREADS) {
        const uint32_t i = i0 + tid;
        const uint32_t p = i < n2 ? blobs2[b2 + i].parent - b1 : 0xffffffffu;
        s_par[tid] = p;
        __syncthreads();
        if (p < n1) {
            uint32_t rank = s_px[p];
            for (int t = 0; t < tid; ++t) rank += s_par[t] == p;
            const uint32_t pos = s_cnt[p] + 1 + rank;
            if (pos < c.per_frame) sq[pos] = (int32_t)(e2 + i);
        }
        __syncthreads();
        if (p < n1) atomicAdd(&s_px[p], 1u);
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();

    // stable compaction of the sequence: committed first, then big
    int32_t* ord = order + (size_t)f * c.per_frame;
    uint32_t n_commit = 0, n_big = 0, n_out = 0;
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t base = pass == 0 ? 0 : n_commit, found = 0;
        for (uint32_t s0 = 0; s0 < n_seq; s0 += PRE_THREADS) {
            const uint32_t s = s0 + tid;
            int32_t e = -1;
            uint32_t d = 255, parent = 0xffffffffu;                           // parent: the entry's detect blob, index in the frame
            if (s < n_seq) {
                e = sq[s];
                if ((uint32_t)e - e1 < n1) parent = (uint32_t)e - e1;
                else if ((uint32_t)e - e2 < n2) parent = blobs2[b2 + ((uint32_t)e - e2)].parent - b1;
                if (parent < n1) d = decision[e];
            }
            const bool take = d == (uint32_t)pass;
            uint32_t total;
            const uint32_t ex = block_flag_scan(take, s_w, total);
            if (take) {
                ord[base + found + ex] = e;
                if (pass == 1) presumed[b1 + parent] = 2;                     // split_expectation(2, false), PrefilterBlobs.cpp:223
            }
            found += total;
            if (pass == 0) {
                uint32_t t2;
                (void)block_flag_scan(d >= 16 && d != 255, s_w, t2);
                n_out += t2;
            }
        }
        if (pass == 0) n_commit = found; else n_big = found;
    }
    if (tid == 0) { counts[4 * f + 0] = (int32_t)n_commit; counts[4 * f + 1] = (int32_t)n_big; counts[4 * f + 2] = (int32_t)n_out; counts[4 * f + 3] = 0; }
}

}  // namespace

int launch_prefilter(trexhip_ctx* ctx, const trexhip_prefilter_params* pp, const trexhip_prefilter_tables* tb, uint8_t* d_decision, int32_t* d_order,
                     int32_t* d_counts, int32_t* d_presumed_nr) {
    const int n = ctx->tables.valid_n;
    const size_t cap = (size_t)ctx->p.max_batch * ctx->p.max_blobs, per_frame = 2 * (size_t)ctx->p.max_blobs;
    PreCfg c = {};
    c.W = ctx->cfg.W; c.H = ctx->cfg.H; c.B = n; c.invert = ctx->batch_invert; c.method = pp->method; c.thr = pp->track_threshold; c.thr2 = pp->track_threshold_2;
    c.n_ranges = pp->n_ranges; c.sqcm = ctx->cfg.sqcm; c.ratio_lo = pp->threshold_ratio_range[0]; c.ratio_hi = pp->threshold_ratio_range[1];
    c.min_start = -1; c.max_end = -1;
    for (int i = 0; i < pp->n_ranges; ++i) {
        const double a = pp->size_ranges[2 * i], b = pp->size_ranges[2 * i + 1];
        c.ranges[2 * i] = a; c.ranges[2 * i + 1] = b;
        if (c.min_start == -1 || a < c.min_start) c.min_start = a;
        if (c.max_end == -1 || b > c.max_end) c.max_end = b;
    }
    c.n_inc = tb ? tb->n_include_shapes : 0; c.n_inc_pts = tb ? tb->n_include_points : 0;
    c.n_ign = tb ? tb->n_ignore_shapes : 0; c.n_ign_pts = tb ? tb->n_ignore_points : 0;
    c.n_bdx = tb && tb->d_ignore_bdx ? tb->n_ignore_bdx : 0;
    c.cap = (uint32_t)cap; c.per_frame = (uint32_t)per_frame; c.mb = (uint32_t)ctx->p.max_blobs;
    // total detect blobs of the fetched batch (every frame's pooled slice, flagged ones included): the whole of d_presumed_nr is zeroed
    uint32_t n1max = 1, total1 = 0;
    for (int f = 0; f < n; ++f) {
        total1 = std::max(total1, ctx->tables.h_info[f].blob_begin + ctx->tables.h_info[f].n_blobs);
        if (ctx->tables.h_info[f].flags) continue;
        n1max = std::max(n1max, ctx->tables.h_info[f].n_blobs);
    }
    total1 = std::min<uint32_t>(std::max(total1, ctx->tables.h_totals[0]), (uint32_t)cap);
    c.n1max = n1max;
    const size_t lds = sizeof(float2) * (size_t)(c.n_inc_pts + c.n_ign_pts) + sizeof(int) * (size_t)(c.n_inc + c.n_ign + 2) + 3 * sizeof(uint32_t) * (size_t)n1max;
    if (lds + 4096 > PRE_LDS_LIMIT) {
        set_error("trexhip_prefilter_device: the shape tables and " + std::to_string(n1max) + " blobs of one frame do not fit the workgroup's LDS");
        return TREXHIP_E_CAPACITY;
    }
    if (!ctx->attr_prefilter) {
        TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pre_decide<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PRE_LDS_LIMIT - 4096));
        TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pre_decide<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PRE_LDS_LIMIT - 4096));
        ctx->attr_prefilter = true;
    }
    if (int rc = ctx->pre.reserve(ctx, sizeof(int32_t) * (2 * cap + (size_t)ctx->p.max_batch * per_frame), "trexhip_prefilter_device")) return rc;
    int32_t* d_count2_own = ctx->pre.as<int32_t>();
    int32_t* d_seq = d_count2_own + 2 * cap;
    int32_t* d_count2 = tb && tb->d_second_count ? tb->d_second_count : d_count2_own;
    hipStream_t s = ctx->stream;

    // the re-threshold of Tracker.cpp:833-837, by the code path of trexhip_rethreshold_device
    int rc = launch_rethreshold(ctx, pp->track_threshold, pp->method, pp->size_ranges, pp->n_ranges, nullptr);
    if (rc) return rc;
    Pass2& q = ctx->pass2;
    TH_CHECK_HIP(hipMemsetAsync(d_decision, 255, 2 * cap, s));
    TH_CHECK_HIP(hipMemsetAsync(d_order, 255, sizeof(int32_t) * (size_t)n * per_frame, s));
    if (total1) TH_CHECK_HIP(hipMemsetAsync(d_presumed_nr, 0, sizeof(int32_t) * total1, s));
    if (c.thr2 > 0 || (tb && tb->d_second_count)) TH_CHECK_HIP(hipMemsetAsync(d_count2, 255, sizeof(int32_t) * 2 * cap, s));   // PRE_NOT_COUNTED
    const float2* ip = tb ? reinterpret_cast<const float2*>(tb->d_include_points) : nullptr;
    const float2* gp = tb ? reinterpret_cast<const float2*>(tb->d_ignore_points) : nullptr;
    const int* io = tb ? tb->d_include_offsets : nullptr;
    const int* go = tb ? tb->d_ignore_offsets : nullptr;
    const uint32_t* bx = tb ? tb->d_ignore_bdx : nullptr;
    const int* bo = bx ? tb->d_ignore_bdx_offsets : nullptr;
    const uint32_t* tot1 = ctx->tables.d_totals;
    if (c.thr2 > 0) {
        hipLaunchKernelGGL(k_pre_decide<1>, dim3(n), dim3(PRE_THREADS), lds, s, c, ctx->tables.d_info, ctx->tables.d_blobs, q.tables.d_info, q.tables.d_blobs, ip, io, gp, go, bx, bo,
                           d_count2, d_seq, d_decision, d_order, d_counts, d_presumed_nr);
        const unsigned waves_wanted = (unsigned)std::min<size_t>((size_t)total1 + cap, (size_t)ctx->n_cus * 32);
        hipLaunchKernelGGL(k_pre_count2, dim3((waves_wanted + 3) / 4), dim3(PRE_THREADS), 0, s, c, ctx->d_frames, ctx->d_bg, ctx->tables.d_info, ctx->tables.d_blob_frame,
                           ctx->tables.d_blobs, ctx->tables.d_runs, tot1, q.tables.d_info, q.tables.d_blob_frame, q.tables.d_blobs, q.tables.d_runs, q.tables.d_totals, d_count2);
    }
    hipLaunchKernelGGL(k_pre_decide<0>, dim3(n), dim3(PRE_THREADS), lds, s, c, ctx->tables.d_info, ctx->tables.d_blobs, q.tables.d_info, q.tables.d_blobs, ip, io, gp, go, bx, bo,
                       d_count2, d_seq, d_decision, d_order, d_counts, d_presumed_nr);
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

}  // namespace trexhip

extern "C" {

void trexhip_default_prefilter_params(trexhip_prefilter_params* p) {
    if (!p) return;
    *p = trexhip_prefilter_params();
    p->track_threshold = 15;             // core/default_config.cpp track_threshold
    p->method = 0;                       // track_threshold_is_absolute true (core/default_config.cpp:941)
    p->track_threshold_2 = 0;
    p->threshold_ratio_range[0] = 0.5f;
    p->threshold_ratio_range[1] = 1.0f;
    p->n_ranges = 0;
}

int trexhip_prefilter_device(trexhip_ctx* ctx, const trexhip_prefilter_params* pp, const trexhip_prefilter_tables* tb, uint8_t* d_decision,
                             int32_t* d_order, int32_t* d_counts, int32_t* d_presumed_nr) {
    using trexhip::set_error;
    if (!ctx || !pp || !d_decision || !d_order || !d_counts || !d_presumed_nr) { set_error("trexhip_prefilter_device: null argument"); return TREXHIP_E_INVALID; }
    if (pp->n_ranges > 8) { set_error("trexhip_prefilter_device: more than 8 ranges in track_size_filter"); return TREXHIP_E_UNSUPPORTED; }
    if (pp->n_ranges < 0 || pp->track_threshold < 0 || pp->track_threshold > 255 || pp->track_threshold_2 < 0 || pp->track_threshold_2 > 255) {
        set_error("trexhip_prefilter_device: thresholds must lie in 0..255 and n_ranges must not be negative"); return TREXHIP_E_INVALID;
    }
    if (tb) {
        if (tb->n_include_shapes > trexhip::PRE_MAX_SHAPES || tb->n_ignore_shapes > trexhip::PRE_MAX_SHAPES || tb->n_include_points > trexhip::PRE_MAX_POINTS ||
            tb->n_ignore_points > trexhip::PRE_MAX_POINTS) {
            set_error("trexhip_prefilter_device: more than 64 shapes or 4096 points in track_include / track_ignore"); return TREXHIP_E_UNSUPPORTED;
        }
        if (tb->n_include_shapes < 0 || tb->n_ignore_shapes < 0 || tb->n_include_points < 0 || tb->n_ignore_points < 0 || tb->n_ignore_bdx < 0 ||
            (tb->n_include_shapes && (!tb->d_include_points || !tb->d_include_offsets)) || (tb->n_ignore_shapes && (!tb->d_ignore_points || !tb->d_ignore_offsets)) ||
            (tb->d_ignore_bdx && !tb->d_ignore_bdx_offsets)) {
            set_error("trexhip_prefilter_device: bad shape / bdx tables"); return TREXHIP_E_INVALID;
        }
    }
    int rc = trexhip::rethreshold_prepare(ctx, "trexhip_prefilter_device", pp->method, pp->size_ranges, pp->n_ranges);
    if (rc) return rc;
    return trexhip::launch_prefilter(ctx, pp, tb, d_decision, d_order, d_counts, d_presumed_nr);
}

}  // extern "C"
