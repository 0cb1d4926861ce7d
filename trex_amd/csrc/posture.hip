// posture.hip -- posture::calculate_posture for every blob of a segmented batch, one wave per blob.
//
// Replaces Application/src/tracker/tracking/Posture.cpp:305-399 (one threshold iteration: the blob table handed in is
// either the detect table or the re-threshold table, i.e. threshold_get_biggest_blob is done by the caller choosing
// the sub-blob) and Outline.cpp.  The phases of k_posture, in the order of the functions below:
//   load_runs, build_bitmap                                       the blob's runs, row table and (narrow blobs) occupancy words in LDS
//   trace_parallel / trace_sequential   (pixel::find_outer_points, commons)   outline on the half-pixel lattice (definition: DESIGN.md section 2)
//   resample                       Outline.cpp:724-766            sequential float walk, lane 0, same operation order
//   smooth                         Outline.cpp:330-378            one lane per point
//   orient_clockwise, eft, curvature_tail_head   Outline::offset_to_middle, Outline.cpp:454-718   clockwise test, EFT(order) -> inverse, curvature, tail/head
//   walk                           Outline::calculate_midline, Outline.cpp:768-868   two-pointer walk
// Everything of one blob lives in the wave's slice of LDS (WaveBlob: runs, row table, two point buffers, curvature, arc length).
// The float pipeline is compiled without FMA contraction (-ffp-contract=off in the Makefile) so resample / smooth /
// walk reproduce the CPU operation order; the transcendental part (EFT) agrees to float rounding.
#include "internal.h"
#include <algorithm>

namespace trexhip {

static constexpr int P_NP = 4096;      // largest max_points (one blob per workgroup beyond ~1300: the LDS of a CU holds fewer large blobs)
static constexpr int P_NR = 2048;      // runs per blob held in LDS
static constexpr int P_ROWS = 1022;    // rows per blob
// bytes of LDS per wave for a given point capacity: two point buffers, curvature, arc length, runs, row table
// (nr / nrows = line and row capacity of this launch: the host sizes them to the largest blob of the fetched table, so that more
// blobs fit into a CU's LDS -- the kernel is a chain of LDS / memory latencies and lives on the number of blobs in flight)
__host__ __device__ constexpr int posture_wave_lds(int np, int nr, int nrows) { return np * 8 * 2 + np * 4 * 2 + nr * 4 + (nrows + 2) * 4; }
// bytes of LDS per lane group of k_posture_walk: the outline and one index pair per segment
__host__ __device__ constexpr size_t posture_walk_lds(int max_points) { return (size_t)max_points * 8 + ((((size_t)max_points / 2 + 1) * 4 + 7) & ~(size_t)7); }
// candidates per search of the two-pointer walk over an outline of n points
__host__ __device__ inline int walk_max_offset(float offset, int n) { float mo = offset * (float)n; if (mo < 3.0f) mo = 3.0f; return (int)mo; }

struct PostureCfg {
    float outline_resample; int smooth_samples, smooth_step, approximate;
    float curvature_range_ratio, midline_walk_offset; int max_points;
    int nr_cap, rows_cap;            // <= P_NR, P_ROWS
    int walk_group;                  // bits 8 / 16: blobs whose two-pointer walk searches at most 8 / 16 candidates leave the walk to k_posture_walk<8> / <16>
};

// The wave's slice of LDS.  Six arrays (np = max_points): bufA, bufB float2 [np]; s_curv, s_t float [np]; s_runs uint32 [nr_cap]; s_row int [rows_cap + 2].
// The outline lives in bufA / bufB by turns (pts = the current one, other = the spare one); every other phase borrows what is idle:
//   view               array                                    written by                       dead after
//   runs, row table    s_runs, s_row                            load_runs                        the trace
//   bitmap()           s_curv, s_t (2 words per row, <= np)     build_bitmap                     the trace (trace_parallel: rows <= np / 2, it ends inside s_curv)
//   side_base()        bufA as uint16 [4 rows + 1]              trace_parallel, numbering        trace_parallel's successor pass (the points then take bufA)
//   side_owner()       second half of bufB as uint16 [np]       trace_parallel, numbering        the successor pass (pointer jumping then takes it)
//   jump(0), jump(1)   bufB as uint32 [np] each                 trace_parallel, successor pass   trace_parallel's emission of the points
//   side_geo()         s_t as uint32 [np]                       trace_parallel, successor pass   trace_parallel's emission of the points
//   traced points      bufA                                     the trace                        resample (writes bufB = pts)
//   smooth_weights()   s_curv [33]                              smooth                           smooth
//   arc()              s_t [np]                                 eft                              eft
//   closing_phase()    s_curv [2]: cos, sin at boundary n       eft                              eft
//   coef()             s_curv + 2 as [16][4] (harmonic 1 at 4)  eft, orders above three          eft
//   phases             other: cos, sin at boundaries 0 .. n-1   eft                              eft's inverse (writes the new outline there)
//   curvature          s_curv [np]                              curvature_tail_head              curvature_tail_head
//   pairs()            s_curv as uint32 [np / 2 + 1]            walk                             walk
struct WaveBlob {
    float2 *bufA, *bufB, *pts, *other;
    float *s_curv, *s_t;
    uint32_t* s_runs; int* s_row;
    int np;
    __device__ __forceinline__ WaveBlob(uint8_t* plds, int wave, const PostureCfg& P) : np(P.max_points) {
        uint8_t* base = plds + (size_t)wave * posture_wave_lds(np, P.nr_cap, P.rows_cap);
        bufA = reinterpret_cast<float2*>(base); bufB = bufA + np;
        s_curv = reinterpret_cast<float*>(bufB + np); s_t = s_curv + np;
        s_runs = reinterpret_cast<uint32_t*>(s_t + np); s_row = reinterpret_cast<int*>(s_runs + P.nr_cap);
        pts = bufB; other = bufA;                                   // resample leaves the outline in bufB
    }
    __device__ __forceinline__ void swap() { float2* t = pts; pts = other; other = t; }
    __device__ __forceinline__ uint32_t* bitmap() const { return reinterpret_cast<uint32_t*>(s_curv); }
    __device__ __forceinline__ uint16_t* side_base() const { return reinterpret_cast<uint16_t*>(bufA); }
    __device__ __forceinline__ uint32_t* jump(int k) const { return reinterpret_cast<uint32_t*>(bufB) + k * np; }
    __device__ __forceinline__ uint16_t* side_owner() const { return reinterpret_cast<uint16_t*>(jump(1)); }
    __device__ __forceinline__ uint32_t* side_geo() const { return reinterpret_cast<uint32_t*>(s_t); }
    __device__ __forceinline__ float* smooth_weights() const { return s_curv; }
    __device__ __forceinline__ float* arc() const { return s_t; }
    __device__ __forceinline__ float* closing_phase() const { return s_curv; }
    __device__ __forceinline__ float* coef() const { return s_curv + 2; }
    __device__ __forceinline__ uint32_t* pairs() const { return reinterpret_cast<uint32_t*>(s_curv); }
};

// where the blob lies: rows y0 .. y1, bitmap column 0 at x = bx0, output coordinates relative to (ox, oy)
struct BlobBox { int n_runs, y0, y1, rows, bx0, ox, oy; bool use_bm; };

// ---- wave primitives: each lane's values in and out in registers ----
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// inclusive scan over the 64 lanes: lane l gets v[0] + ... + v[l], added in the order of the doubling steps (the CPU restatement's order for floats)
template <typename T> __device__ __forceinline__ T wave_scan_inclusive(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T t = __shfl_up(v, d); if (lane >= d) v += t; }
    return v;
}
__device__ __forceinline__ int wave_scan_inclusive_max(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d); if (lane >= d && t > v) v = t; }
    return v;
}
// (value, index) of the FIRST extremum over aligned groups of LANES lanes, in every lane of the group: the smallest (MAX: largest) value and among
// equal values the lowest index -- what a sequential scan with a strict comparison keeps.  Comparisons only: the order of the steps does not matter.
template <int LANES, bool MAX> __device__ __forceinline__ void first_extremum(float& v, int& idx) {
#pragma unroll
    for (int d = 1; d < LANES; d <<= 1) {
        const float ov = __shfl_xor(v, d); const int oi = __shfl_xor(idx, d);
        if ((MAX ? ov > v : ov < v) || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}
template <int LANES> __device__ __forceinline__ void first_min(float& v, int& idx) { first_extremum<LANES, false>(v, idx); }
__device__ __forceinline__ void first_max(float& v, int& idx) { first_extremum<64, true>(v, idx); }

// sin / cos of the EFT phases: the same operations in the same order as the CPU restatement's det_sincosf (tests' checker) (Cody-Waite reduction by pi/2 in three
// pieces, degree-7 / degree-8 polynomials on [-pi/4, pi/4]; this file is compiled with -ffp-contract=off): bit-identical to the CPU restatement,
// which the library sincosf (and glibc's on the other side) was not -- the tail / head choice flipped at near-ties of the curvature peaks.
__device__ __forceinline__ void det_sincosf(const float x, float& sn, float& cs) {
    const float kf = floorf(x * 0.636619772f + 0.5f);
    const int k = (int)kf;
    float r = x - kf * 1.5703125f;
    r = r - kf * 4.837512969970703125e-4f;
    r = r - kf * 7.54978995489188216e-8f;
    const float z = r * r;
    float ps = -1.9515295891e-4f; ps = ps * z + 8.3321608736e-3f; ps = ps * z - 1.6666654611e-1f;
    const float s0 = r + r * z * ps;
    float pc = 2.443315711809948e-5f; pc = pc * z - 1.388731625493765e-3f; pc = pc * z + 4.166664568298827e-2f;
    const float c0 = (1.0f - 0.5f * z) + z * z * pc;
    const bool swap = k & 1;
    const float a = swap ? c0 : s0, b = swap ? s0 : c0;
    sn = (k & 2) ? -a : a;
    cs = ((k + 1) & 2) ? -b : b;
}
// phase (h - 1) theta -> h theta from (c1, s1) = cos, sin of theta: h = 2 by the doubling form, h >= 3 by angle addition (c, s = harmonic h - 1 in, h out)
__device__ __forceinline__ void harmonic_advance(float& c, float& s, const float c1, const float s1, const int h) {
    float cn, sn;
    if (h == 2) { cn = c1 * c1 - s1 * s1; sn = 2.0f * (s1 * c1); } else { cn = c * c1 - s * s1; sn = s * c1 + c * s1; }
    c = cn; s = sn;
}
// distance a - b of a walk's candidate and its key; a distance that is not below FLT_MAX never wins (the sequential `len < min_d` rule)
__device__ __forceinline__ void walk_candidate(const float2 a, const float2 b, const int key, float& len, int& idx) {
    const float ddx = a.x - b.x, ddy = a.y - b.y;
    len = sqrtf(ddx * ddx + ddy * ddy); idx = key;
    if (!(len < 3.402823466e38f)) { len = 3.402823466e38f; idx = 0x7fffffff; }
}
// one midline segment from its two outline points: midpoint, distance between the points, distance midpoint - left point
__device__ __forceinline__ float4 midline_segment(const float2 pt_r, const float2 pt_l) {
    const float lx = pt_r.x - pt_l.x, ly = pt_r.y - pt_l.y;
    const float mx = pt_l.x + lx * 0.5f, my = pt_l.y + ly * 0.5f;
    return make_float4(mx, my, sqrtf(lx * lx + ly * ly), sqrtf((mx - pt_l.x) * (mx - pt_l.x) + (my - pt_l.y) * (my - pt_l.y)));
}

// ---- the phases of k_posture.  Unless a function says otherwise its scalar arguments and results are wave-uniform and all 64 lanes call it. ----

__device__ __forceinline__ void load_runs(const WaveBlob& v, const trexhip_run* __restrict__ rr, const BlobBox& b, const int lane) {
    uint32_t* s_runs = v.s_runs; int* s_row = v.s_row;
    for (int i = lane; i < b.n_runs; i += 64) {
        const trexhip_run q = rr[i];
        s_runs[i] = (uint32_t)q.x0 | ((uint32_t)q.x1 << 16);
        if (i == 0 || rr[i - 1].y != q.y) s_row[q.y - b.y0] = i;
    }
    if (lane == 0) s_row[b.rows] = b.n_runs;
    __builtin_amdgcn_wave_barrier();
}

// blobs at most 64 pixels wide (b.use_bm): one 64-bit occupancy word per row makes the membership test of the boundary walk a single LDS read
__device__ __forceinline__ void build_bitmap(const WaveBlob& v, const trexhip_run* __restrict__ rr, const BlobBox& b, const int lane) {
    uint32_t* bm = v.bitmap();
    for (int i = lane; i < b.rows * 2; i += 64) bm[i] = 0u;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < b.n_runs; i += 64) {
        const trexhip_run q = rr[i];
        const int a = (int)q.x0 - b.bx0, len = (int)q.x1 - (int)q.x0 + 1;
        const unsigned long long m = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << a;
        if ((uint32_t)m) atomicOr(&bm[2 * (q.y - b.y0)], (uint32_t)m);
        if ((uint32_t)(m >> 32)) atomicOr(&bm[2 * (q.y - b.y0) + 1], (uint32_t)(m >> 32));
    }
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool inside(const WaveBlob& v, const BlobBox& b, int x, int y) {
    if (y < b.y0 || y > b.y1) return false;
    if (!b.use_bm) {
        const uint32_t* s_runs = v.s_runs; const int* s_row = v.s_row;
        for (int i = s_row[y - b.y0]; i < s_row[y - b.y0 + 1]; ++i) {
            const uint32_t r = s_runs[i];
            if (x >= (int)(r & 0xffffu) && x <= (int)(r >> 16)) return true;
        }
        return false;
    }
    const int xr = x - b.bx0;
    if ((unsigned)xr >= 64u) return false;
    return (v.bitmap()[2 * (y - b.y0) + (xr >> 5)] >> (xr & 31)) & 1u;
}

// ---- outline on the half-pixel lattice ----
// The boundary is a permutation of directed pixel sides: side k of pixel p (k = 0 top, moving +x; 1 right, +y; 2 bottom, -x;
// 3 left, -y; the blob on the right hand) is followed by the left-turn side of the pixel ahead-left if that pixel is set, else
// the same side of the pixel ahead, else the next side of p itself -- exactly the turn rule of trace_sequential.  All
// sides are numbered (per row and direction: popcounts of bit masks), every lane computes successors, pointer jumping ranks
// the cycle through the start side (top side of the first pixel), and each side emits its two points at its rank: ~100
// dependent steps of one lane become ~10 short passes of the whole wave.  Needs the one-word-per-row bitmap, rows <= max_points/2 and at most max_points
// sides (holes included); anything else returns false and takes the sequential walk.  true: nt (points in bufA, 0 beyond the capacity) and status are set in every lane.
__device__ __forceinline__ bool trace_parallel(const WaveBlob& v, const BlobBox& b, const int lane, int& nt, int& status) {
    const int NPc = v.np, rows = b.rows;
    if (!(b.use_bm && rows * 2 <= NPc)) return false;
    const uint32_t* bm = v.bitmap();
    uint16_t* base16 = v.side_base();                                  // first side id per (row, direction)
    uint32_t* jmp0 = v.jump(0);                                        // next id | hops to the last side << 16, double buffered
    uint32_t* jmp1 = v.jump(1);
    uint32_t* geo = v.side_geo();                                      // x | row << 6 | direction << 16
    auto row64 = [&](int yr) -> unsigned long long {
        return (yr < 0 || yr >= rows) ? 0ull : ((unsigned long long)bm[2 * yr] | ((unsigned long long)bm[2 * yr + 1] << 32));
    };
    auto side_mask = [&](int yr, int k) -> unsigned long long {
        const unsigned long long R = row64(yr);
        return k == 0 ? R & ~row64(yr - 1) : (k == 1 ? R & ~(R >> 1) : (k == 2 ? R & ~row64(yr + 1) : R & ~(R << 1)));
    };
    const int items = rows * 4;
    uint32_t running = 0;
    for (int i0 = 0; i0 < items; i0 += 64) {
        const int it = i0 + lane;
        const uint32_t cnt = it < items ? (uint32_t)__popcll(side_mask(it >> 2, it & 3)) : 0u;
        const uint32_t incl = wave_scan_inclusive(cnt, lane);
        if (it < items) base16[it] = (uint16_t)(running + incl - cnt);
        running += (uint32_t)__shfl((int)incl, 63);
    }
    const int E = (int)running;
    if (E > NPc) return false;
    // one lane per SIDE (a lane per (row, direction) would walk up to 60 sides of a horizontal animal's top row while the others idle): the
    // (row, direction) item that owns side id e is the last one whose first id is <= e -- items write their number at their first id, a
    // running maximum fills the rest --, and the side is the (e - first id)-th set bit of the item's mask
    uint16_t* owner = v.side_owner();
    for (int e = lane; e < E; e += 64) owner[e] = 0;
    if (lane == 0) base16[items] = (uint16_t)E;
    __builtin_amdgcn_wave_barrier();
    for (int it = lane; it < items; it += 64) { const uint16_t b0 = base16[it]; if (base16[it + 1] != b0) owner[b0] = (uint16_t)it; }
    __builtin_amdgcn_wave_barrier();
    int carry = 0;
    for (int e0 = 0; e0 < E; e0 += 64) {
        const int e = e0 + lane;
        int it = wave_scan_inclusive_max(e < E ? (int)owner[e] : 0, lane);
        if (carry > it) it = carry;
        carry = __shfl(it, 63);
        if (e >= E) continue;
        const int yr = it >> 2, k = it & 3;
        const unsigned long long m = side_mask(yr, k);
        int kk = e - (int)base16[it];                                       // the kk-th set bit of m
        uint32_t w = (uint32_t)m; int xr = 0;
        { const int c = __popc(w); if (kk >= c) { kk -= c; w = (uint32_t)(m >> 32); xr = 32; } }
        { const int c = __popc(w & 0xffffu); if (kk >= c) { kk -= c; w >>= 16; xr += 16; } }
        { const int c = __popc(w & 0xffu); if (kk >= c) { kk -= c; w >>= 8; xr += 8; } }
        { const int c = __popc(w & 0xfu); if (kk >= c) { kk -= c; w >>= 4; xr += 4; } }
        { const int c = __popc(w & 0x3u); if (kk >= c) { kk -= c; w >>= 2; xr += 2; } }
        if (kk >= (int)(w & 1u)) xr += 1;
        const int ddx = k == 0 ? 1 : (k == 2 ? -1 : 0), ddy = k == 1 ? 1 : (k == 3 ? -1 : 0);
        const int kl = (k + 3) & 3;
        const int lx = kl == 0 ? 1 : (kl == 2 ? -1 : 0), ly = kl == 1 ? 1 : (kl == 3 ? -1 : 0);
        int tx = xr + ddx + lx, ty = yr + ddy + ly, tk = kl;                     // ahead-left: turn left
        if (!((unsigned)tx < 64u && ((row64(ty) >> tx) & 1ull))) {
            tx = xr + ddx; ty = yr + ddy; tk = k;                                // ahead: straight on
            if (!((unsigned)tx < 64u && ((row64(ty) >> tx) & 1ull))) { tx = xr; ty = yr; tk = (k + 1) & 3; }   // turn right
        }
        const uint32_t tid = (uint32_t)base16[ty * 4 + tk] + (uint32_t)__popcll(side_mask(ty, tk) & ((1ull << tx) - 1ull));
        // the side whose successor is the start side (id 0: first top side of the first row) ends the cycle
        jmp0[e] = tid == 0u ? (uint32_t)e : (tid | (1u << 16));
        geo[e] = (uint32_t)xr | ((uint32_t)yr << 6) | ((uint32_t)k << 16);      // x < 64, row < 1024
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t* cur = jmp0; uint32_t* oth = jmp1;
    for (int span = 1; span < E; span <<= 1) {
        for (int e = lane; e < E; e += 64) {
            const uint32_t a = cur[e], w = cur[a & 0xffffu];
            oth[e] = (w & 0xffffu) | (((a >> 16) + (w >> 16)) << 16);
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t* t = cur; cur = oth; oth = t;
    }
    const uint32_t first = cur[0];
    const int len = (int)(first >> 16) + 1;                                     // sides on the outer cycle
    nt = 2 * len;
    if (nt > NPc) { status = 2; nt = 0; return true; }                          // an outline beyond the capacity reports no points at all
    for (int e = lane; e < E; e += 64) {
        const uint32_t a = cur[e];
        if ((a & 0xffffu) != (first & 0xffffu)) continue;                    // a hole's boundary
        const int pos = (int)(first >> 16) - (int)(a >> 16);
        const uint32_t g = geo[e];
        const int xr = (int)(g & 0x3fu), yr = (int)((g >> 6) & 0x3ffu), k = (int)(g >> 16);
        const int vx = 2 * (xr + b.bx0 - b.ox) + ((k == 1 || k == 2) ? 1 : -1), vy = 2 * (yr + b.y0 - b.oy) + ((k >= 2) ? 1 : -1);   // doubled, relative to the origin
        const int ddx = k == 0 ? 1 : (k == 2 ? -1 : 0), ddy = k == 1 ? 1 : (k == 3 ? -1 : 0);
        v.bufA[2 * pos] = make_float2(0.5f * (float)vx, 0.5f * (float)vy);
        v.bufA[2 * pos + 1] = make_float2(0.5f * (float)(vx + ddx), 0.5f * (float)(vy + ddy));
    }
    return true;
}

// the same boundary by one lane: lane 0 walks, then nt and status are republished from lane 0 to every lane
__device__ __forceinline__ void trace_sequential(const WaveBlob& v, const BlobBox& b, const int lane, int& nt, int& status) {
    if (lane == 0) {
        const int fx = (int)(v.s_runs[0] & 0xffffu);
        const int sx = 2 * fx - 1, sy = 2 * b.y0 - 1, ox = b.ox, oy = b.oy;
        int vx = sx, vy = sy, dx = 1, dy = 0, k = 0;
        do {
            if (k + 2 > v.np) { status = 2; break; }
            v.bufA[k++] = make_float2(0.5f * (float)(vx - 2 * ox), 0.5f * (float)(vy - 2 * oy));
            v.bufA[k++] = make_float2(0.5f * (float)(vx + dx - 2 * ox), 0.5f * (float)(vy + dy - 2 * oy));
            vx += 2 * dx; vy += 2 * dy;
            const int lx = dy, ly = -dx, rx = -dy, ry = dx;
            if (inside(v, b, (vx + dx + lx) / 2, (vy + dy + ly) / 2)) { dx = lx; dy = ly; }
            else if (inside(v, b, (vx + dx + rx) / 2, (vy + dy + ry) / 2)) { }
            else { dx = rx; dy = ry; }
        } while (!(vx == sx && vy == sy && dx == 1 && dy == 0));
        nt = status ? 0 : k;                            // an outline beyond the capacity reports no points at all
    }
    nt = __shfl(nt, 0); status = __shfl(status, 0);
}

// Outline::resample (Outline.cpp:724-766): nt traced points in bufA -> n points in bufB.  Every segment of the lattice outline is exactly 0.5
// long, so when 2 * resample distance is a whole number k all of the reference's float arithmetic is exact and it emits the start point of every
// k-th segment: done by all lanes, n and status wave-uniform throughout.  Any other distance takes the sequential walk (same operation order as
// the reference) in lane 0, and n and status are republished from lane 0 afterwards.
__device__ __forceinline__ void resample(const WaveBlob& v, const float rd, const int lane, const int nt, int& n, int& status) {
    const float2* bufA = v.bufA; float2* bufB = v.bufB;
    const int cap = v.np;
    const float k2 = rd * 2.0f;
    const bool lattice = rd > 0.f && k2 == floorf(k2) && k2 <= 1024.f;
    if (!status && lattice && nt > 1) {
        const int k = (int)k2;
        n = nt / k;
        if (n > cap) { status = 2; n = 0; }
        else {
            for (int jx = lane; jx < n; jx += 64) bufB[jx] = bufA[(jx + 1) * k - 1];
            if (n == 0) status = 1;
        }
    } else if (lane == 0) {
        if (!status) {
            if (rd <= 0.f || nt <= 1) { for (int i = 0; i < nt; ++i) bufB[i] = bufA[i]; n = nt; }
            else {
                float walked = 0.0f;
                for (int i = 0; i < nt && !status; ++i) {
                    int i1 = i + 1; if (i1 >= nt) i1 -= nt;
                    const float2 pt0 = bufA[i], pt1 = bufA[i1];
                    const float lxn = pt1.x - pt0.x, lyn = pt1.y - pt0.y;
                    const float len = sqrtf(lxn * lxn + lyn * lyn);
                    walked += len;
                    const float percent = len / rd;
                    float wp = walked / rd;
                    int offset = 0;
                    while (wp >= 1.0f) {
                        const float tt = (float)((double)offset * 1.0 / (double)percent);
                        if (n >= cap) { status = 2; break; }
                        bufB[n++] = make_float2(pt0.x + lxn * tt, pt0.y + lyn * tt);
                        offset++;
                        walked -= rd;
                        wp -= 1.0f;
                    }
                }
            }
            if (!status && n == 0) status = 1;
        }
    }
    if (!(lattice && nt > 1)) { n = __shfl(n, 0); status = __shfl(status, 0); }
    __builtin_amdgcn_wave_barrier();
}

// smooth_outline (Outline.cpp:330-378): triangular weights over +-range*step
__device__ __forceinline__ void smooth(WaveBlob& v, const PostureCfg& P, const int n, const int lane) {
    if (!(P.smooth_samples > 0 && n > P.smooth_samples)) return;
    const float step_row = (float)P.smooth_samples * (float)P.smooth_step;
    // the normalised weights w[s] / sum once per blob: lane s holds weight s, the sum runs over them in the reference's order
    float* s_w = v.smooth_weights();
    int nw = 0; float sum = 0.f, mine = 0.f;
    for (int i = (int)-step_row; i <= step_row && nw < 33; i += P.smooth_step) { const float val = (step_row - fabsf((float)i)) / step_row; sum += val; if (nw == lane) mine = val; ++nw; }
    if (lane < nw) s_w[lane] = mine / sum;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < n; i += 64) {
        float2 pt = make_float2(0.f, 0.f); int s = 0;
        for (int j = (int)((float)i - step_row); (float)j <= (float)i + step_row; j += P.smooth_step) {
            int idx = j; while (idx < 0) idx += n; while (idx >= n) idx -= n;
            const float ww = s_w[s < 32 ? s : 32]; ++s;
            const float2 q = v.pts[idx];
            pt.x += q.x * ww; pt.y += q.y * ww;
        }
        v.other[i] = pt;
    }
    __builtin_amdgcn_wave_barrier();
    v.swap();
}

// offset_to_middle's clockwise test: a counter-clockwise outline is reversed
__device__ __forceinline__ void orient_clockwise(WaveBlob& v, const int n, const int lane) {
    float part = 0.f;
    for (int i = lane; i < n; i += 64) { const float2 a = v.pts[i], q = v.pts[i + 1 == n ? 0 : i + 1]; part += a.x * q.y - q.x * a.y; }
    if (wsum(part) < 0.f) {
        for (int i = lane; i < n; i += 64) v.other[i] = v.pts[n - 1 - i];
        __builtin_amdgcn_wave_barrier();
        v.swap();
    }
}

// ---- EFT (order) -> inverse at n uniform parameters around the centre ----
// what segment i gives to every harmonic: the gradient of the outline over its arc length and cos, sin of the first harmonic's phase at its two ends
struct EftTerm { float gx, gy; float2 c0, c1; };
// a lane's partial sums of the coefficients a b c d for the three harmonics of one sweep
struct EftSums { float a[3], b[3], c[3], d[3]; };
// false: a segment of no length, it adds nothing
__device__ __forceinline__ bool eft_segment_term(const WaveBlob& v, const int i, const int n, const float csE, const float snE, EftTerm& t) {
    const float* s_t = v.arc();
    const float2 a = v.pts[i], q = v.pts[i + 1 == n ? 0 : i + 1];
    const float t0 = i > 0 ? s_t[i - 1] : 0.f, t1 = s_t[i];
    const float dt = t1 - t0;
    if (dt <= 0.f) return false;
    t.c0 = v.other[i]; t.c1 = (i + 1 < n) ? v.other[i + 1] : make_float2(csE, snE);
    const float ddx = q.x - a.x, ddy = q.y - a.y;
    t.gx = ddx / dt; t.gy = ddy / dt;
    return true;
}
// One sweep over the segments for harmonics hb, hb + 1, hb + 2 (those <= last): s.a[k] .. s.d[k] = this lane's partial sums of harmonic hb + k.  Term i goes
// to partial sum i % 64 in order of i, the caller combines the partials by the xor butterfly (wsum): the order the CPU restatement follows too.  The
// phases follow the recurrence of harmonic_advance, always started at harmonic 1: a sweep recomputes it up to hb, which gives the values a single
// sweep over all harmonics would have had (no iterations when hb == 1).
__device__ __forceinline__ void eft_sweep(const WaveBlob& v, const int n, const int lane, const int hb, const int last, EftSums& s) {
    const float csE = v.closing_phase()[0], snE = v.closing_phase()[1];
    for (int i = lane; i < n; i += 64) {
        EftTerm t;
        if (!eft_segment_term(v, i, n, csE, snE, t)) continue;
        float c0h = t.c0.x, s0h = t.c0.y, c1h = t.c1.x, s1h = t.c1.y;
        for (int h = 2; h <= hb; ++h) { harmonic_advance(c0h, s0h, t.c0.x, t.c0.y, h); harmonic_advance(c1h, s1h, t.c1.x, t.c1.y, h); }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int h = hb + k;
            if (h <= last) {
                if (k > 0) { harmonic_advance(c0h, s0h, t.c0.x, t.c0.y, h); harmonic_advance(c1h, s1h, t.c1.x, t.c1.y, h); }
                const float dc = c1h - c0h, ds = s1h - s0h;
                s.a[k] += t.gx * dc; s.b[k] += t.gx * ds; s.c[k] += t.gy * dc; s.d[k] += t.gy * ds;
            }
        }
    }
}
// coefficients and inverse.  REG (orders 1 .. 3): one sweep, the coefficients stay in registers and the inverse is unrolled; else (4 .. 15, a uint8_t
// without an upper bound in the reference, core/default_config.cpp:888) three harmonics per sweep and the coefficients in coef().  The same sums per
// harmonic and the same recurrence in both.
template <bool REG>
__device__ __forceinline__ void eft_series(const WaveBlob& v, const int order, const int n, const int lane, const float cx, const float cy, const float T) {
    const float PI = 3.14159265358979323846f;
    float ca[4][4];                                           // REG: [harmonic 1..3][a b c d]
    float* coef = v.coef();
    for (int hb = 1; hb <= (REG ? 1 : order); hb += 3) {
        EftSums s = {};
        eft_sweep(v, n, lane, hb, order, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int h = hb + k;
            if (h <= order) {
                const float kf = T / (2.0f * (float)(h * h) * PI * PI);
                const float va = kf * wsum(s.a[k]), vb = kf * wsum(s.b[k]), vc = kf * wsum(s.c[k]), vd = kf * wsum(s.d[k]);
                if constexpr (REG) { ca[h][0] = va; ca[h][1] = vb; ca[h][2] = vc; ca[h][3] = vd; }
                else if (lane == 0) { coef[4 * h] = va; coef[4 * h + 1] = vb; coef[4 * h + 2] = vc; coef[4 * h + 3] = vd; }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < n; i += 64) {
        const float tt = (float)i / (float)n;
        float x = cx, y = cy;
        float s1, c1;
        det_sincosf(2.0f * PI * (float)1 * tt, s1, c1);
        float ch = c1, sh = s1;
        auto harmonic = [&](const int h) {
            if (h > 1) harmonic_advance(ch, sh, c1, s1, h);
            if constexpr (REG) { x += ca[h][0] * ch + ca[h][1] * sh; y += ca[h][2] * ch + ca[h][3] * sh; }
            else { x += coef[4 * h] * ch + coef[4 * h + 1] * sh; y += coef[4 * h + 2] * ch + coef[4 * h + 3] * sh; }
        };
        if constexpr (REG) {
#pragma unroll
            for (int h = 1; h <= 3; ++h) if (h <= order) harmonic(h);
        } else {
            for (int h = 1; h <= order; ++h) harmonic(h);
        }
        v.other[i] = make_float2(x, y);
    }
}
__device__ __forceinline__ void eft(WaveBlob& v, const int order, const int n, const int lane) {
    // the centre: Outline.cpp:502-505 adds the points IN ORDER, and a float sum is its order -- every lane walks the same sequence (LDS broadcasts)
    // (eight points per iteration: the loads of a block are independent of the running sums, only the adds are the chain)
    float cx = 0.f, cy = 0.f;
    int ic = 0;
    for (; ic + 8 <= n; ic += 8) {
        float2 a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = v.pts[ic + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) { cx += a[k].x; cy += a[k].y; }
    }
    for (; ic < n; ++ic) { const float2 a = v.pts[ic]; cx += a.x; cy += a.y; }
    cx /= (float)n; cy /= (float)n;
    // cumulative arc length (wave scan over chunks of 64 segments + a running carry; the tests' CPU restatement follows exactly this order):
    // s_t[i] = arc length at the END of segment i
    float* s_t = v.arc();
    float run = 0.f;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        float dt = 0.f;
        if (i < n) { const float2 a = v.pts[i], q = v.pts[i + 1 == n ? 0 : i + 1]; dt = sqrtf((q.x - a.x) * (q.x - a.x) + (q.y - a.y) * (q.y - a.y)); }
        const float incl = wave_scan_inclusive(dt, lane);
        if (i < n) s_t[i] = run + incl;
        run += __shfl(incl, 63);
    }
    __builtin_amdgcn_wave_barrier();
    const float T = s_t[n - 1];
    const float PI = 3.14159265358979323846f;
    // cos / sin of the FIRST harmonic's phase at every segment boundary once (boundary i = the start of segment i = the end of segment i - 1;
    // boundary n closes the curve: it goes to closing_phase()), kept in the spare point buffer.  The higher harmonics follow by harmonic_advance:
    // one sin / cos per boundary instead of one per harmonic -- the CPU restatement does the same operations in the same order
    for (int i = lane; i <= n; i += 64) {
        float sn, cs;
        det_sincosf(2.0f * PI * (float)1 * (i > 0 ? s_t[i - 1] : 0.f) / T, sn, cs);
        if (i < n) v.other[i] = make_float2(cs, sn);
        else { v.closing_phase()[0] = cs; v.closing_phase()[1] = sn; }
    }
    __builtin_amdgcn_wave_barrier();
    if (order > 3) eft_series<false>(v, order, n, lane, cx, cy, T);
    else eft_series<true>(v, order, n, lane, cx, cy, T);
    __builtin_amdgcn_wave_barrier();
    v.swap();
}

// curvature, tail = highest peak, head = the peak farthest from it along the outline (0x7fffffff: none).  false: no curvature peak at all.
__device__ __forceinline__ bool curvature_tail_head(const WaveBlob& v, const float range_ratio, const int n, const int lane, int& tail, int& head) {
    const float2* pts = v.pts; float* s_curv = v.s_curv;
    int r = (int)(range_ratio * (float)n); if (r < 1) r = 1;
    for (int i = lane; i < n; i += 64) {
        // (i -+ r) mod n; r < n except for range ratios >= 1
        const int im = r < n ? (i - r < 0 ? i - r + n : i - r) : ((i - r) % n + n) % n, ip = r < n ? (i + r >= n ? i + r - n : i + r) : (i + r) % n;
        const float2 p1 = pts[im], p2 = pts[i], p3 = pts[ip];
        const float cr = (p2.x - p1.x) * (p3.y - p2.y) - (p2.y - p1.y) * (p3.x - p2.x);
        const float d12 = (p2.x - p1.x) * (p2.x - p1.x) + (p2.y - p1.y) * (p2.y - p1.y);
        const float d23 = (p3.x - p2.x) * (p3.x - p2.x) + (p3.y - p2.y) * (p3.y - p2.y);
        const float d13 = (p3.x - p1.x) * (p3.x - p1.x) + (p3.y - p1.y) * (p3.y - p1.y);
        const float den = sqrtf(d12 * d23 * d13);
        s_curv[i] = den > 0.f ? fabsf(2.0f * cr / den) : 0.0f;
    }
    __builtin_amdgcn_wave_barrier();
    float best = -1.f; tail = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const float c0 = s_curv[i == 0 ? n - 1 : i - 1], c1 = s_curv[i], c2 = s_curv[i + 1 == n ? 0 : i + 1];
        if (c1 > c0 && c1 >= c2 && c1 > best) { best = c1; tail = i; }        // per lane: first index of its maximum
    }
    first_max(best, tail);
    if (tail == 0x7fffffff || best < 0.f) return false;
    float maxd = 0.f; head = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const float c0 = s_curv[i == 0 ? n - 1 : i - 1], c1 = s_curv[i], c2 = s_curv[i + 1 == n ? 0 : i + 1];
        if (!(c1 > c0 && c1 >= c2)) continue;
        float dd;
        if (i >= tail) dd = fminf(fabsf((float)(i - tail)), fabsf((float)(i - tail - n)));
        else dd = fminf(fabsf((float)(tail - i)), fabsf((float)(tail - i - n)));
        if (dd > maxd) { maxd = dd; head = i; }
    }
    first_max(maxd, head);
    return true;
}

// The two-pointer walk (Outline.cpp:790-857) while a search holds at most 64 candidates: control flow is wave-uniform, the max_offset candidates of
// each search are evaluated one per lane and reduced to the FIRST minimum (the sequential `len < min_d` rule) over RED lanes (a power of two >=
// max_offset).  The kernel is bound by instruction issue, so the loop only keeps what the next iteration depends on: the pair of outline indices of
// every segment goes to pairs() (right index, 0xffff = none, | left index << 16).  -> the number of segments walked.
template <int RED>
__device__ __forceinline__ int walk_pairs(const float2* pts, uint32_t* s_pair, const int L, const int max_offset, const int seg_cap, const int lane) {
    const float BIG = 3.402823466e38f;
    int idx_r = 1, idx_l = -1, ns = 0;
    while (idx_r < L + idx_l) {
        // the three LDS reads of an iteration depend only on the indices of the previous one: one round trip, not four
        const bool cand_r = lane < max_offset && idx_r + lane < L, cand_l = lane < max_offset && idx_l - lane > -L;
        const float2 pl0 = pts[L + idx_l];
        const float2 cr = cand_r ? pts[idx_r + lane] : make_float2(0.f, 0.f);
        const float2 cl = cand_l ? pts[L + idx_l - lane] : make_float2(0.f, 0.f);
        float len = BIG; int idx = 0x7fffffff;
        if (cand_r) walk_candidate(cr, pl0, idx_r + lane, len, idx);
        first_min<RED>(len, idx);
        // the winner's point comes out of its lane's registers (v_readlane), and the state stays wave-uniform
        float2 pt_r = make_float2(0.f, 0.f);
        uint32_t used_r = 0xffffu;
        const int idx0 = __builtin_amdgcn_readfirstlane(idx);
        if (idx0 != 0x7fffffff) {
            const int wl = idx0 - __builtin_amdgcn_readfirstlane(idx_r);
            pt_r.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cr.x), wl));
            pt_r.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cr.y), wl));
            idx_r = idx0; used_r = (uint32_t)idx0;
        }
        float len2 = BIG; int key = 0x7fffffff;
        if (cand_l) walk_candidate(pt_r, cl, lane, len2, key);
        first_min<RED>(len2, key);
        const int key0 = __builtin_amdgcn_readfirstlane(key);
        if (key0 != 0x7fffffff) idx_l -= key0;
        if (lane == 0 && ns < seg_cap) s_pair[ns] = used_r | ((uint32_t)(L + idx_l) << 16);
        ++ns;
        idx_r++; idx_l--;
    }
    return ns;
}
// the segments of the pairs a walk left: two square roots each, by all lanes
__device__ __forceinline__ void segments_from_pairs(const float2* pts, const uint32_t* s_pair, const int nseg, float4* so, const int first, const int stride) {
    for (int i = first; i < nseg; i += stride) {
        const uint32_t pr = s_pair[i];
        const float2 pt_r = (pr & 0xffffu) == 0xffffu ? make_float2(0.f, 0.f) : pts[pr & 0xffffu];
        so[i] = midline_segment(pt_r, pts[pr >> 16]);
    }
}
// the walk of one blob by its wave: the n points of v.pts (tail at 0) -> so, at most max_points / 2 + 1 segments; -> the number of segments walked
__device__ __forceinline__ int walk(const WaveBlob& v, const PostureCfg& P, const int n, const int lane, float4* so) {
    const float2* pts = v.pts;
    const int L = n, max_offset = walk_max_offset(P.midline_walk_offset, L), seg_cap = P.max_points / 2 + 1;
    if (max_offset <= 64) {
        uint32_t* s_pair = v.pairs();
        int ns;
        if (max_offset <= 4) ns = walk_pairs<4>(pts, s_pair, L, max_offset, seg_cap, lane);
        else if (max_offset <= 8) ns = walk_pairs<8>(pts, s_pair, L, max_offset, seg_cap, lane);
        else if (max_offset <= 16) ns = walk_pairs<16>(pts, s_pair, L, max_offset, seg_cap, lane);
        else ns = walk_pairs<64>(pts, s_pair, L, max_offset, seg_cap, lane);
        __builtin_amdgcn_wave_barrier();
        segments_from_pairs(pts, s_pair, ns < seg_cap ? ns : seg_cap, so, lane, 64);
        return ns;
    }
    // more candidates than lanes (midline_walk_offset * points > 64): a search takes its candidates i = 0 .. max_offset - 1 in passes of 64
    const float BIG = 3.402823466e38f;
    auto search = [&](auto candidate) -> int {                     // -> the key of the first minimum, 0x7fffffff: none
        int best_key = 0x7fffffff; float best = BIG;
        for (int i0 = 0; i0 < max_offset; i0 += 64) {
            float len = BIG; int key = 0x7fffffff;
            if (i0 + lane < max_offset) candidate(i0 + lane, len, key);
            first_min<64>(len, key);
            if (key != 0x7fffffff && len < best) { best = len; best_key = key; }    // strict `<`: earlier candidates keep ties
        }
        return best_key;
    };
    int idx_r = 1, idx_l = -1, ns = 0;
    while (idx_r < L + idx_l) {
        float2 pt_r = make_float2(0.f, 0.f); float2 pt_l = pts[L + idx_l];
        const int kr = search([&](int i, float& len, int& key) { if (idx_r + i < L) walk_candidate(pts[idx_r + i], pt_l, idx_r + i, len, key); });
        if (kr != 0x7fffffff) { pt_r = pts[kr]; idx_r = kr; }
        const int kl = search([&](int i, float& len, int& key) { if (idx_l - i > -L) walk_candidate(pt_r, pts[L + idx_l - i], i, len, key); });
        if (kl != 0x7fffffff) { idx_l -= kl; pt_l = pts[L + idx_l]; }
        if (lane == 0 && ns < seg_cap) so[ns] = midline_segment(pt_r, pt_l);
        ++ns;
        idx_r++; idx_l--;
    }
    return ns;
}

__global__ __launch_bounds__(256) void k_posture(const PostureCfg P, const trexhip_frame_info* __restrict__ info,
                                                 const uint32_t* __restrict__ blob_frame, const trexhip_blob* __restrict__ blobs,
                                                 const trexhip_run* __restrict__ runs, int n_blobs, int B,
                                                 float2* __restrict__ out_outline, float4* __restrict__ out_segments,
                                                 trexhip_posture_info* __restrict__ out_info,
                                                 const int32_t* __restrict__ sel, const trexhip_blob* __restrict__ origin) {
    extern __shared__ __attribute__((aligned(16))) uint8_t plds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bi = blockIdx.x * (int)(blockDim.x >> 6) + wave;   // 4, 2 or 1 blobs per workgroup (LDS per blob)
    if (bi >= n_blobs) return;
    trexhip_posture_info res = {};
    auto finish = [&](int status) { if (lane == 0) { res.status = status; out_info[bi] = res; } };
    // sel: output slot bi takes blob sel[bi] of the table (negative: nothing to do for this slot); origin: the blob whose bounds().pos()
    // the coordinates are relative to (the ORIGINAL blob when a thresholded sub-blob is traced, Posture.cpp:336)
    const int si = sel ? sel[bi] : bi;
    if (si < 0) return;
    const uint32_t f = blob_frame[si];
    bool ok = f < (uint32_t)B;
    trexhip_frame_info fi = {};
    if (ok) { fi = info[f]; ok = fi.flags == 0; }
    if (!ok) { finish(1); return; }
    const trexhip_blob Bl = blobs[si];
    BlobBox box;
    box.n_runs = (int)Bl.n_runs; box.y0 = Bl.y0; box.y1 = Bl.y1; box.rows = box.y1 - box.y0 + 1; box.bx0 = Bl.x0;
    if (box.n_runs == 0) { finish(1); return; }
    if (box.n_runs > P.nr_cap || box.rows > P.rows_cap) { finish(2); return; }
    box.ox = origin ? (int)origin[bi].x0 : (int)Bl.x0; box.oy = origin ? (int)origin[bi].y0 : (int)Bl.y0;
    box.use_bm = (int)Bl.x1 - (int)Bl.x0 < 64 && box.rows <= P.max_points;
    WaveBlob v(plds, wave, P);
    const trexhip_run* rr = runs + fi.run_begin + Bl.run_begin;
    load_runs(v, rr, box, lane);
    if (box.use_bm) build_bitmap(v, rr, box, lane);

    int n = 0, status = 0;
    if (!trace_parallel(v, box, lane, res.n_traced, status)) trace_sequential(v, box, lane, res.n_traced, status);
    __builtin_amdgcn_wave_barrier();
    resample(v, P.outline_resample, lane, res.n_traced, n, status);
    if (status) { finish(status); return; }
    smooth(v, P, n, lane);
    orient_clockwise(v, n, lane);
    if (P.approximate > 0) eft(v, P.approximate, n, lane);       // 1 .. 15 (the launch refuses more)
    float2* oo = out_outline + (size_t)bi * P.max_points;
    int tail, head;
    if (!curvature_tail_head(v, P.curvature_range_ratio, n, lane, tail, head)) {
        // no curvature peak: the outline stays available (first_outline fallback, Posture.cpp:361-368)
        for (int i = lane; i < n; i += 64) oo[i] = v.pts[i];
        res.n_outline = n; finish(3);
        return;
    }
    // rotate so that the tail is point 0 (Outline.cpp:707); this is the outline the caller gets
    for (int i = lane; i < n; i += 64) { const float2 p = v.pts[i + tail >= n ? i + tail - n : i + tail]; v.other[i] = p; oo[i] = p; }
    __builtin_amdgcn_wave_barrier();
    v.swap();
    res.n_outline = n; res.tail_index = 0;
    res.head_index = head == 0x7fffffff ? -1 : ((head - tail) % n + n) % n;
    if (n <= 1) { finish(1); return; }
    // the walk keeps 3 .. a few lanes of a wave busy (max_offset candidates per search) and is bound by instruction issue: blobs whose searches fit a
    // small lane group are finished by k_posture_walk, several blobs per wave (n_segments = -G / 8 of the smallest launched group that holds them)
    const int m0 = walk_max_offset(P.midline_walk_offset, n);
    const int tag = ((P.walk_group & 8) && m0 <= 8) ? -1 : (((P.walk_group & 16) && m0 <= 16) ? -2 : 0);
    if (tag) { res.n_segments = tag; finish(0); return; }
    const int ns = walk(v, P, n, lane, out_segments + (size_t)bi * (P.max_points / 2 + 1));
    res.n_segments = ns; finish(ns <= 2 ? 4 : 0);
}

// ------------------------------------------------------------------------------------------------
// k_posture_walk: the two-pointer walk of k_posture (Outline.cpp:790-857) for the blobs it tagged (n_segments == -G / 8), 64 / G blobs per wave.
// The walk is a chain of ~40 dependent steps per blob with 3 .. a few candidates per search: one blob per wave leaves the vector unit nearly
// empty and the phase bound by instruction issue.  Here a group of G lanes owns a blob -- its outline (written by k_posture, tail at point 0)
// in the group's LDS, the max_offset <= G candidates of a search one per lane -- and a step costs the wave ~100 instructions for 64 / G blobs:
// the minimum distance over the group is three or four v_min_u32 with a DPP operand (distances are >= +0, their bit patterns order like the
// values), the FIRST minimum (the sequential `len < min_d` rule) is the lowest set bit of the group's part of a ballot, and the winning point
// is read back from LDS.  The same float operations in the same order as the in-kernel walk; groups whose blobs take fewer steps idle.
// ------------------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ uint32_t dpp_min_u32(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, CTRL, 0xf, 0xf, false);
    return o < v ? o : v;
}
template <int G> __device__ __forceinline__ uint32_t group_min_u32(uint32_t v) {
    v = dpp_min_u32<0xB1>(v);                              // quad_perm [1,0,3,2]
    v = dpp_min_u32<0x4E>(v);                              // quad_perm [2,3,0,1]
    if (G >= 8) v = dpp_min_u32<0x141>(v);                 // row_half_mirror: the other quad of the 8
    if (G >= 16) v = dpp_min_u32<0x140>(v);                // row_mirror: the other half of the 16
    return v;
}
template <int G>
__global__ __launch_bounds__(64) void k_posture_walk(const float walk_offset, const int max_points, const int n_blobs, const float2* __restrict__ outline,
                                                     float4* __restrict__ out_segments, trexhip_posture_info* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) uint8_t wlds[];
    constexpr int BPW = 64 / G;
    const int lane = threadIdx.x, g = lane % G, grp = lane / G, gbase = lane - g;
    const int bi = blockIdx.x * BPW + grp;
    const int seg_cap = max_points / 2 + 1;
    const size_t per = posture_walk_lds(max_points);
    float2* pts = reinterpret_cast<float2*>(wlds + (size_t)grp * per);
    uint32_t* s_pair = reinterpret_cast<uint32_t*>(pts + max_points);
    int L = 0;                                             // 0: not this kernel's blob (every lane stays, the wave loads the outlines together)
    if (bi < n_blobs) {
        const trexhip_posture_info pi = info[bi];
        if (pi.status == 0 && pi.n_segments == -(G / 8)) L = pi.n_outline;
    }
    // ---- the outlines: the whole wave loads one blob's points at a time, the first 128 points of all blobs in flight together
    {
        float2 v0[BPW], v1[BPW];
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const int Lb = __builtin_amdgcn_readlane(L, b * G);
            const float2* src = outline + (size_t)(blockIdx.x * BPW + b) * max_points;
            v0[b] = lane < Lb ? src[lane] : make_float2(0.f, 0.f);
            v1[b] = lane + 64 < Lb ? src[lane + 64] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int b = 0; b < BPW; ++b) {
            const int Lb = __builtin_amdgcn_readlane(L, b * G);
            float2* dst = reinterpret_cast<float2*>(wlds + (size_t)b * per);
            if (lane < Lb) dst[lane] = v0[b];
            if (lane + 64 < Lb) dst[lane + 64] = v1[b];
            if (Lb > 128) {
                const float2* src = outline + (size_t)(blockIdx.x * BPW + b) * max_points;
                for (int i = 128 + lane; i < Lb; i += 64) dst[i] = src[i];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();                       // one wave: its LDS operations stay in order
    int idx_r = 1, idx_l = -1, ns = 0;
    const int max_offset = walk_max_offset(walk_offset, L);   // <= G (k_posture's own test)
    const uint32_t BIGU = 0x7f7fffffu;                     // FLT_MAX: "no candidate"
    const bool in_search = g < max_offset;
    while (idx_r < L + idx_l) {
        const int il = L + idx_l;
        const bool cand_r = in_search && idx_r + g < L, cand_l = in_search && il - g > 0;
        const float2 pl0 = pts[il];
        const float2 cr = pts[cand_r ? idx_r + g : 0];
        const float2 cl = pts[cand_l ? il - g : 0];
        uint32_t lb = BIGU;
        {
            const float ddx = cr.x - pl0.x, ddy = cr.y - pl0.y;
            const uint32_t b = __builtin_bit_cast(uint32_t, sqrtf(ddx * ddx + ddy * ddy));
            if (cand_r && b < BIGU) lb = b;                // NaN / inf patterns are above FLT_MAX: !(len < FLT_MAX) never wins
        }
        const uint32_t m1 = group_min_u32<G>(lb);
        const uint64_t w1 = __ballot(lb == m1 && lb != BIGU);
        const uint32_t g1 = (uint32_t)(w1 >> gbase) & ((1u << G) - 1u);
        float2 pt_r = make_float2(0.f, 0.f);
        uint32_t used_r = 0xffffu;
        if (g1) { idx_r += __builtin_ctz(g1); used_r = (uint32_t)idx_r; pt_r = pts[idx_r]; }   // the same in every lane of the group
        uint32_t lb2 = BIGU;
        {
            const float ddx = pt_r.x - cl.x, ddy = pt_r.y - cl.y;
            const uint32_t b = __builtin_bit_cast(uint32_t, sqrtf(ddx * ddx + ddy * ddy));
            if (cand_l && b < BIGU) lb2 = b;
        }
        const uint32_t m2 = group_min_u32<G>(lb2);
        const uint64_t w2 = __ballot(lb2 == m2 && lb2 != BIGU);
        const uint32_t g2 = (uint32_t)(w2 >> gbase) & ((1u << G) - 1u);
        if (g2) idx_l -= __builtin_ctz(g2);
        if (g == 0 && ns < seg_cap) s_pair[ns] = used_r | ((uint32_t)(L + idx_l) << 16);
        ++ns;
        idx_r++; idx_l--;
    }
    if (L == 0) return;
    __builtin_amdgcn_wave_barrier();
    segments_from_pairs(pts, s_pair, ns < seg_cap ? ns : seg_cap, out_segments + (size_t)bi * seg_cap, g, G);
    if (g == 0) { info[bi].n_segments = ns; info[bi].status = ns <= 2 ? 4 : 0; }
}

// which lane groups of k_posture_walk a launch uses (bits 8, 16): groups of 8 take the blobs whose searches fit them (twice the blobs per wave),
// groups of 16 the rest up to 16 candidates and are not launched when the parameters cannot need them; searches of more than 16 candidates stay
// inside k_posture, and so does everything when the outlines of a wave's blobs do not fit 64 KB of LDS.  (Groups of 4 -- 16 blobs per wave, 40 KB
// of LDS at 256 points -- leave one wave per SIMD and measured slower than groups of 8: 62 vs 50 us per 25 600 blobs.)
static int posture_walk_groups(const trexhip_posture_params* pp) {
    const size_t per = posture_walk_lds(pp->max_points);
    const bool a8 = per * 8 <= 64 * 1024, a16 = per * 4 <= 64 * 1024;
    return (a8 ? 8 : 0) | (a16 && (walk_max_offset(pp->midline_walk_offset, pp->max_points) > 8 || !a8) ? 16 : 0);
}

struct PostureOut { float2* outline; float4* segments; trexhip_posture_info* info; };

template <int G> static void launch_posture_walk(hipStream_t s, const PostureCfg& P, int n_blobs, const PostureOut& out) {
    constexpr int bpw = 64 / G;
    const size_t lds = posture_walk_lds(P.max_points) * (size_t)bpw;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_posture_walk<G>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_posture_walk<G>), dim3((unsigned)((n_blobs + bpw - 1) / bpw)), dim3(64), lds, s, P.midline_walk_offset, P.max_points, n_blobs,
                       (const float2*)out.outline, out.segments, out.info);
}

// How one posture launch is shaped: the kernel's settings, the LDS line / row capacities, blobs per workgroup and LDS bytes.
struct PosturePlan {
    PostureCfg P;
    int wpb, lds_bytes;
    // Line / row capacity from the fetched host table `t` (the kernel's full capacity when it is not at hand).  sub_blobs = false: the table's own
    // blobs are traced -- their lines; blobs beyond P_NR / P_ROWS report status 2 anyway and do not count.  sub_blobs = true (the retry loop): their
    // thresholded sub-blobs -- the parent's rows at most, more lines only where a line splits: twice the parent's, an ESTIMATE (k_auto_step, widen()).
    PosturePlan(const trexhip_posture_params* pp, const BlobTables& t, int n_blobs, bool sub_blobs)
        : P{pp->outline_resample, pp->outline_smooth_samples, pp->outline_smooth_step, pp->outline_approximate,
            pp->outline_curvature_range_ratio, pp->midline_walk_offset, pp->max_points, P_NR, P_ROWS, posture_walk_groups(pp)} {
        if (t.h_blobs && t.fetched) {
            uint32_t mr = 1, mrows = 1;
            for (int i = 0; i < n_blobs; ++i) {
                const trexhip_blob& b = t.h_blobs[i];
                const uint32_t lines = sub_blobs ? std::min<uint32_t>(b.n_runs * 2u, (uint32_t)P_NR) : b.n_runs;
                if (lines > (uint32_t)P_NR) continue;
                const uint32_t rws = (uint32_t)(b.y1 - b.y0 + 1);
                if (rws <= (uint32_t)P_ROWS) { mr = std::max(mr, lines); mrows = std::max(mrows, rws); }
            }
            P.nr_cap = (int)std::min<uint32_t>((mr + 31u) & ~31u, (uint32_t)P_NR);
            P.rows_cap = (int)std::min<uint32_t>((mrows + 29u) / 32u * 32u + 30u, (uint32_t)P_ROWS);      // (rows_cap + 2) * 4 stays 16-byte friendly
        }
        size();
    }
    // the kernel's real limits (fewer blobs per CU)
    void widen() { P.nr_cap = P_NR; P.rows_cap = P_ROWS; size(); }
    // blobs per workgroup: 4 while their LDS fits a CU comfortably, else 2 or 1 (large max_points / large blobs)
    void size() {
        const int wave_lds = posture_wave_lds(P.max_points, P.nr_cap, P.rows_cap);
        wpb = 4;
        while (wpb > 1 && wpb * wave_lds > 150 * 1024) wpb >>= 1;
        lds_bytes = wpb * wave_lds;
    }
};

// k_posture and the walk kernels for output slots 0 .. n-1 on the context's stream, inside the posture stage timer
static int launch_posture(trexhip_ctx* ctx, const PosturePlan& plan, const BlobTables& t, int n, const PostureOut& out, const int32_t* sel, const trexhip_blob* origin) {
    if (plan.lds_bytes > ctx->attr_posture_bytes) {
        TH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_posture), hipFuncAttributeMaxDynamicSharedMemorySize, plan.lds_bytes));
        ctx->attr_posture_bytes = plan.lds_bytes;
    }
    stage_begin(ctx, TREXHIP_STAGE_POSTURE);
    hipLaunchKernelGGL(k_posture, dim3((n + plan.wpb - 1) / plan.wpb), dim3(plan.wpb * 64), plan.lds_bytes, ctx->stream, plan.P, t.d_info, t.d_blob_frame, t.d_blobs, t.d_runs,
                       n, ctx->tables.valid_n, out.outline, out.segments, out.info, sel, origin);
    if (plan.P.walk_group & 8) launch_posture_walk<8>(ctx->stream, plan.P, n, out);
    if (plan.P.walk_group & 16) launch_posture_walk<16>(ctx->stream, plan.P, n, out);
    stage_end(ctx, TREXHIP_STAGE_POSTURE);
    return TREXHIP_OK;
}

// the settings both entry points accept, and a fetched batch to work on (both report under the single pass's name)
static int validate_posture_params(const trexhip_ctx* ctx, const trexhip_posture_params* pp) {
    if (pp->max_points < 8 || pp->max_points > P_NP || (pp->max_points & 1)) { set_error("trexhip_posture_device: max_points must be even and in 8..4096"); return TREXHIP_E_INVALID; }
    if (pp->outline_smooth_samples < 0 || pp->outline_smooth_samples * (pp->outline_smooth_step > 0 ? pp->outline_smooth_step : 1) > 16 || pp->outline_smooth_step < 1) {
        set_error("trexhip_posture_device: outline_smooth_samples*outline_smooth_step must be <= 16"); return TREXHIP_E_UNSUPPORTED;
    }
    // (outline_approximate is a uint8_t without an upper bound in the reference, core/default_config.cpp:888: up to 15 harmonics here; beyond three
    // the [16][4] coefficients live in the curvature array -- 66 floats)
    if (pp->outline_approximate > 15 || (pp->outline_approximate > 3 && pp->max_points < 128)) {
        set_error("trexhip_posture_device: outline_approximate > 15 (or > 3 with max_points < 128) is not supported"); return TREXHIP_E_UNSUPPORTED;
    }
    // settings whose arithmetic is not built (it lives in the un-vendored commons and nothing in the tree pins it): refuse
    if (pp->posture_closing_steps != 0) { set_error("trexhip_posture_device: posture_closing_steps > 0 is not implemented (closing inside pixel::threshold_get_biggest_blob, Posture.cpp:335)"); return TREXHIP_E_UNSUPPORTED; }
    if (pp->peak_mode != 0) { set_error("trexhip_posture_device: peak_mode = broad is not implemented (needs periodic::find_peaks' peak ranges / integrals, Outline.cpp:627-661); only pointy"); return TREXHIP_E_UNSUPPORTED; }
    if (pp->posture_direction_smoothing < 0) { set_error("trexhip_posture_device: posture_direction_smoothing must not be negative"); return TREXHIP_E_INVALID; }   // (> 1: the caller hands the movement direction to trexhip_midline_movement_device)
    if (!ctx->d_frames || ctx->tables.valid_n == 0 || !ctx->tables.fetched) { set_error("trexhip_posture_device: segment and fetch a batch first"); return TREXHIP_E_INVALID; }
    return TREXHIP_OK;
}

}  // namespace trexhip

using namespace trexhip;

extern "C" int trexhip_posture_device(trexhip_ctx* ctx, int32_t table, const trexhip_posture_params* pp, int32_t n_blobs,
                                      float* d_outline, float* d_segments, trexhip_posture_info* d_info) {
    if (!ctx || !pp || !d_outline || !d_segments || !d_info) { set_error("trexhip_posture_device: null argument"); return TREXHIP_E_INVALID; }
    if (int rc = validate_posture_params(ctx, pp)) return rc;
    if (n_blobs < 0 || (uint32_t)n_blobs > ctx->cfg.pool_blobs) { set_error("trexhip_posture_device: n_blobs outside the blob pool"); return TREXHIP_E_INVALID; }
    if (n_blobs == 0) return TREXHIP_OK;
    if (table == 1) {
        if (!ctx->pass2.allocated || ctx->pass2.tables.valid_n == 0) { set_error("trexhip_posture_device: no re-thresholded batch"); return TREXHIP_E_INVALID; }
    } else if (table != 0) { set_error("trexhip_posture_device: table must be 0 (detect) or 1 (re-threshold)"); return TREXHIP_E_INVALID; }
    const BlobTables& t = table == 0 ? ctx->tables : ctx->pass2.tables;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    if (const int rc = fetch_wait(ctx)) return rc;      // the plan reads the fetched blob table on the host
    const PosturePlan plan(pp, t, n_blobs, false);
    if (int rc = launch_posture(ctx, plan, t, n_blobs, PostureOut{reinterpret_cast<float2*>(d_outline), reinterpret_cast<float4*>(d_segments), d_info}, nullptr, nullptr)) return rc;
    TH_CHECK_HIP(hipGetLastError());
    return TREXHIP_OK;
}

// ---- posture::calculate_posture with its retry loop (Posture.cpp:305-399) ---------------------------------------------------------
// Per detect blob: threshold = track_posture_threshold; repeat { biggest sub-blob at `threshold` (pixel::threshold_get_biggest_blob:
// re-threshold + largest pixel count, the first wins a tie) -> outline relative to the ORIGINAL blob -> resample -> midline; success
// ends the loop; else remember the first outline, threshold += 2, stop when that sub-blob had fewer than max(1, initial / 10) pixels or
// threshold >= track_posture_threshold + 100 }; without success the first outline is returned without a midline (:383-391).
// On the device every round is: one per-blob re-threshold pass over the still active blobs (trexhip_rethreshold_per_blob_device),
// k_auto_pick / k_auto_sel (biggest sub-blob per detect blob by a 64-bit atomic max), k_posture on the selected sub-blobs, k_auto_step
// (one wave per blob: bookkeeping, first-outline copy); the host only reads the number of blobs still active.
namespace trexhip {
// the loop's per-blob state in the context's scratch (ctx->autos)
struct AutoState {
    unsigned long long* best;        // [n] pixels << 32 | ~index of the biggest sub-blob of this round
    float2* first;                   // [n][max_points] the first outline that could be traced
    int32_t *thr, *sel, *first_n, *first_thr, *used, *iters;   // [n] each: threshold of this round (negative: finished), selected sub-blob (-1 none, -2 handled), ...
    uint32_t* active;                // [2] blobs going on to the next threshold, blobs asking for a repeat with full LDS capacities
    static size_t bytes(int n, int max_points) { return (size_t)n * (6 * sizeof(int32_t) + sizeof(unsigned long long) + (size_t)max_points * sizeof(float2)) + 64; }
    static AutoState carve(uint8_t* base, int n, int max_points) {
        AutoState a;
        auto take = [&](size_t each) { uint8_t* p = base; base += (size_t)n * each; return p; };
        a.best = reinterpret_cast<unsigned long long*>(take(8));
        a.first = reinterpret_cast<float2*>(take((size_t)max_points * sizeof(float2)));
        int32_t** const words[6] = {&a.thr, &a.sel, &a.first_n, &a.first_thr, &a.used, &a.iters};
        for (int32_t** w : words) *w = reinterpret_cast<int32_t*>(take(4));
        a.active = reinterpret_cast<uint32_t*>(base);
        return a;
    }
};
__global__ void k_auto_init(const int n, const int tpt, const AutoState a, trexhip_posture_info* info) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    a.thr[b] = tpt; a.first_n[b] = 0; a.first_thr[b] = -1; a.used[b] = -1; a.iters[b] = 0; a.best[b] = 0ull;
    trexhip_posture_info z = {}; z.status = 1; info[b] = z;
}
__global__ void k_auto_pick(const trexhip_blob* __restrict__ sub, const uint32_t* __restrict__ totals2, const uint32_t pool, const int n,
                            unsigned long long* best) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const uint32_t tot = totals2[0] < pool ? totals2[0] : pool;
    if (s >= tot) return;
    const trexhip_blob B = sub[s];
    if (B.parent >= (uint32_t)n || B.n_pixels == 0) return;                       // holes of frames that overflowed carry no parent
    atomicMax(best + B.parent, ((unsigned long long)B.n_pixels << 32) | (unsigned long long)(0xffffffffu - s));   // most pixels, then the lowest index
}
__global__ void k_auto_sel(const int n, const int32_t* thr, const unsigned long long* best, int32_t* sel) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    sel[b] = (thr[b] >= 0 && best[b] != 0ull) ? (int32_t)(0xffffffffu - (uint32_t)best[b]) : -1;
}
__global__ __launch_bounds__(256) void k_auto_step(const int n, const int tpt, const int max_points, const trexhip_blob* __restrict__ detect,
                                                   const trexhip_blob* __restrict__ sub, const AutoState a, float2* outline, trexhip_posture_info* info,
                                                   const int nr_cap, const int rows_cap) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    const int t = a.thr[b];
    if (t < 0) return;
    const int s = a.sel[b];
    if (s == -2) return;                                   // already handled in this round (the round is being repeated with full LDS capacities)
    const uint32_t count = s >= 0 ? (uint32_t)(a.best[b] >> 32) : 0u;
    trexhip_posture_info last = info[b];
    if (s < 0) { trexhip_posture_info z = {}; z.status = 1; last = z; }
    if (s >= 0 && last.status == 2 && (nr_cap < P_NR || rows_cap < P_ROWS)) {
        // the launch's LDS capacities are an ESTIMATE from the parent blobs (a thresholded line can split into more than two); a sub-blob
        // beyond the estimate but within the kernel's real limits is not a failed attempt: leave the blob as it is and ask for a repeat
        const int sr = (int)sub[s].n_runs, srows = sub[s].y1 - sub[s].y0 + 1;
        if ((sr > nr_cap || srows > rows_cap) && sr <= P_NR && srows <= P_ROWS) {
            if (lane == 0) atomicAdd(a.active + 1, 1u);
            return;
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) { a.iters[b] += 1; a.best[b] = 0ull; a.sel[b] = -2; }
    if (s >= 0 && last.status == 0) { if (lane == 0) { a.used[b] = t; a.thr[b] = -1; } return; }      // a midline at the lowest possible threshold
    float2* mine = outline + (size_t)b * max_points;
    float2* keep = a.first + (size_t)b * max_points;
    int fn = a.first_n[b];
    if (s >= 0 && fn == 0 && last.n_outline > 0) {                                    // the first outline that could be traced
        for (int i = lane; i < last.n_outline; i += 64) keep[i] = mine[i];
        fn = last.n_outline;
        if (lane == 0) { a.first_n[b] = fn; a.first_thr[b] = t; }
    }
    const uint32_t initial = detect[b].n_pixels;
    const uint32_t minimum = initial / 10u > 1u ? initial / 10u : 1u;
    const int tn = t + 2;
    if (count < minimum || tn >= tpt + 100) {                                         // give up: the first outline, no midline
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < fn; i += 64) mine[i] = keep[i];
        if (lane == 0) {
            last.n_outline = fn; last.n_segments = 0;
            if (last.status == 0) last.status = 1;
            info[b] = last;
            a.used[b] = fn > 0 ? (a.first_thr[b] >= 0 ? a.first_thr[b] : t) : -1;
            a.thr[b] = -1;
        }
        return;
    }
    if (lane == 0) { a.thr[b] = tn; atomicAdd(a.active, 1u); }
}
}  // namespace trexhip

extern "C" int trexhip_posture_auto_device(trexhip_ctx* ctx, const trexhip_posture_params* pp, int32_t method, int32_t track_posture_threshold,
                                           int32_t n_blobs, float* d_outline, float* d_segments, trexhip_posture_info* d_info,
                                           int32_t* d_threshold_used, int32_t* d_iterations) {
    if (!ctx || !pp || !d_outline || !d_segments || !d_info) { set_error("trexhip_posture_auto_device: null argument"); return TREXHIP_E_INVALID; }
    if (method < 0 || method > 2) { set_error("trexhip_posture_auto_device: method must be 0 (absolute), 1 (sign) or 2 (none)"); return TREXHIP_E_INVALID; }
    if (track_posture_threshold < 0 || track_posture_threshold > 255) { set_error("trexhip_posture_auto_device: track_posture_threshold must be 0..255"); return TREXHIP_E_INVALID; }
    if (int rc = validate_posture_params(ctx, pp)) return rc;
    if (n_blobs < 0 || (uint32_t)n_blobs > ctx->cfg.pool_blobs) { set_error("trexhip_posture_auto_device: n_blobs outside the blob pool"); return TREXHIP_E_INVALID; }
    if (n_blobs == 0) return TREXHIP_OK;
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    const int n = n_blobs, MPt = pp->max_points;
    if (int rc = ctx->autos.reserve(ctx, AutoState::bytes(n, MPt), "trexhip_posture_auto_device")) return rc;
    const AutoState a = AutoState::carve(ctx->autos.as<uint8_t>(), n, MPt);
    const PostureOut out{reinterpret_cast<float2*>(d_outline), reinterpret_cast<float4*>(d_segments), d_info};
    hipStream_t s = ctx->stream;
    const dim3 g256((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_auto_init, g256, dim3(256), 0, s, n, (int)track_posture_threshold, a, d_info);
    if (const int rc = fetch_wait(ctx)) return rc;
    PosturePlan plan(pp, ctx->tables, n, true);
    for (int round = 0; round < 51; ++round) {                        // thresholds t, t+2, ..., below t+100
        int rc = trexhip_rethreshold_per_blob_device(ctx, 0, a.thr, method, nullptr, 0);     // negative entries (finished blobs) are skipped
        if (rc) return rc;
        const BlobTables& q = ctx->pass2.tables;
        hipLaunchKernelGGL(k_auto_pick, dim3((ctx->cfg.pool_blobs + 255u) / 256u), dim3(256), 0, s, q.d_blobs, q.d_totals, ctx->cfg.pool_blobs, n, a.best);
        hipLaunchKernelGGL(k_auto_sel, g256, dim3(256), 0, s, n, a.thr, a.best, a.sel);
        uint32_t still[2] = {0, 0};
        for (int attempt = 0; attempt < 2; ++attempt) {               // attempt 1: only if a sub-blob did not fit the estimated LDS capacities
            TH_CHECK_HIP(hipMemsetAsync(a.active, 0, 8, s));
            if (int rc2 = launch_posture(ctx, plan, q, n, out, a.sel, ctx->tables.d_blobs)) return rc2;
            hipLaunchKernelGGL(k_auto_step, dim3((n + 3) / 4), dim3(256), 0, s, n, (int)track_posture_threshold, MPt, ctx->tables.d_blobs, q.d_blobs, a,
                               out.outline, d_info, plan.P.nr_cap, plan.P.rows_cap);
            TH_CHECK_HIP(hipGetLastError());
            TH_CHECK_HIP(hipMemcpyAsync(still, a.active, 8, hipMemcpyDeviceToHost, s));
            TH_CHECK_HIP(hipStreamSynchronize(s));
            if (still[1] == 0) break;
            plan.widen();                                              // from here on the kernel's real limits
        }
        if (still[0] == 0) break;
    }
    if (d_threshold_used) TH_CHECK_HIP(hipMemcpyAsync(d_threshold_used, a.used, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (d_iterations) TH_CHECK_HIP(hipMemcpyAsync(d_iterations, a.iters, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return TREXHIP_OK;
}

extern "C" void trexhip_default_posture_params(trexhip_posture_params* p) {
    if (!p) return;
    p->outline_resample = 1.0f; p->outline_smooth_samples = 4; p->outline_smooth_step = 1; p->outline_approximate = 3;
    p->outline_curvature_range_ratio = 0.03f; p->midline_walk_offset = 0.025f; p->max_points = 512;
    p->posture_closing_steps = 0; p->peak_mode = 0; p->posture_direction_smoothing = 0;
}
