// visual_field.hip -- every individual's visual field of a batch of frames, on outlines that are already in HBM.
//
// Replaces track::VisualField::calculate, Application/src/tracker/tracking/VisualField.cpp:361-577, as Individual::save_visual_field
// (tracking/Individual.cpp:2887-3010) asks for it once per individual and frame:
//   tesselate_outline        :339-359   (float32 Vec2 arithmetic, N in double)
//   project_angles_1d        :74-94     with correct_angle :67-72
//   plot_projected_line      :96-150    the two-layer depth buffer with its id tests
//   add_line and the loop over the active individuals   :427-496, :526-576
// include/trexhip.h states the rule and the readings of what the reference leaves to commons; tests/visual_field_ref.py restates it.
//
// Three launches on the context's stream:
//   k_vf_check   offsets ascend, every observer names a frame of the call and an entry of that frame; sets the flag the others respect
//   k_vf_tess    one workgroup per entry, shared by every observer of the frame: per-edge insert counts, a workgroup scan, the
//                tessellated double2 list and its length into scratch (max_tess_points per entry); a longer list flags the entry
//   k_vf_cast    one workgroup per (observer, eye), one thread per bin; a thread holds its bin's two layers in registers.  The
//                workgroup walks the frame's entries in order.  All 512 lanes compute one record each (two atan2, the projection,
//                start, end, d, rp, id, hd, fov: 32 bytes) and append the records that reach a bin to LDS in order (wave ballots +
//                prefix counts over the waves); when LDS cannot take another step, every wave walks the waiting records IN ORDER --
//                64 at a time, one ballot of "touches this wave's 64 bins", then the set bits in ascending order -- and each bin
//                thread applies those whose [start, end] holds its bin.  No atomics and no min-reduction: layer 2 is not a function of
//                a minimum, so the per-bin order of the records is the algorithm; skipping a record for a whole wave cannot reorder.
// The cast is compute-bound: two double atan2 per record and eye, then about a dozen VALU instructions per record and wave;
// it reads the tessellated points of one frame, well under a megabyte, out of L2.
#include "internal.h"
#include <cfloat>
#include <cmath>

namespace trexhip {

static constexpr int VF_RES = TREXHIP_VF_RESOLUTION, VF_THREADS = 512, VF_WAVES = VF_THREADS / 64, VF_CHUNK = TREXHIP_VF_CHUNK_RECORDS,
                     VF_LDS = TREXHIP_VF_LDS_RECORDS, VF_TESS_THREADS = 256, VF_MAX_TESS = 1 << 24;
static_assert(VF_RES == VF_THREADS && VF_CHUNK == VF_THREADS && VF_LDS >= 2 * VF_CHUNK && TREXHIP_VF_LAYERS == 2, "one thread per bin and per record of a step");
static constexpr double VF_PI = 3.14159265358979323846, VF_TWO_PI = 2.0 * VF_PI;
static constexpr double VF_FOV_END = 130.0 * (VF_PI / 180.0), VF_FOV_START = -VF_FOV_END, VF_FOV_LEN = VF_FOV_END - VF_FOV_START;   // RADIANS(130)
static constexpr double VF_INVALID = (double)FLT_MAX;

struct VfArgs {
    trexhip_vf_params p;
    const float2* outline; const trexhip_posture_info* info;
    const int32_t* frame_entries; int n_frames;
    const trexhip_vf_entry* entries; int n_entries;
    const trexhip_vf_observer* observers; int n_observers;
    double* depth; int32_t* ids; float2* points; uint8_t* fov; double* hd; int32_t* status;
    uint32_t* flag;        // an argument in device memory was refused: nothing is written
    int32_t* len;          // [n_entries] tessellated length; -1 = the entry is not used, -2 = it exceeds max_tess_points
    int32_t* tail;         // [n_entries] the tail index the entry goes by (head_index with flag bit 0)
    double2* tess;         // [n_entries][max_tess_points]
};

__global__ __launch_bounds__(256) void k_vf_check(const VfArgs A) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t < A.n_frames) {
        const int a = A.frame_entries[t], b = A.frame_entries[t + 1];
        bad = a < 0 || b < a || b > A.n_entries || (t == 0 && a != 0);
    }
    if (t < A.n_observers) {
        const int f = A.observers[t].frame, e = A.observers[t].entry;
        if (f < 0 || f >= A.n_frames) bad = true;
        else bad = bad || e < A.frame_entries[f] || e >= A.frame_entries[f + 1] || e < 0 || e >= A.n_entries;
    }
    if (bad) atomicOr(A.flag, 1u);
}

// one edge of tesselate_outline (:345-354): the unit direction in float32 and the number of points the loop `for (int i = 1; i < N - 1; ++i)`
// inserts, clamped to cap + 1
__device__ __forceinline__ int vf_edge(float px, float py, float x, float y, double max_distance, int cap, float& dx, float& dy) {
    dx = x - px; dy = y - py;
    const float L = sqrtf(dx * dx + dy * dy);
    int cnt = 0;
    if ((double)L > max_distance) {
        dx /= L; dy /= L;
        const double N = (double)L / max_distance + 0.5, lim = N - 1;
        if (lim > 1) cnt = lim > (double)cap + 2.0 ? cap + 1 : (int)ceil(lim) - 1;      // the integers i with 1 <= i < lim
    }
    return cnt;
}

__global__ __launch_bounds__(VF_TESS_THREADS) void k_vf_tess(const VfArgs A) {
    __shared__ unsigned long long s_part[VF_TESS_THREADS];
    if (*A.flag) return;
    const int e = blockIdx.x, tid = threadIdx.x;
    const trexhip_vf_entry ent = A.entries[e];
    int n = 0, T = -1;
    if (ent.posture_row >= 0) {
        const trexhip_posture_info pi = A.info[ent.posture_row];
        n = pi.n_outline;
        T = (ent.flags & 1) ? pi.head_index : pi.tail_index;
    }
    if (ent.posture_row < 0 || n <= 0 || T == -1) {                                    // :552
        if (tid == 0) { A.len[e] = -1; A.tail[e] = -1; }
        return;
    }
    if (n > A.p.max_points) {                                                           // more points than a row holds: no such outline; flagged like a capacity
        if (tid == 0) { A.len[e] = -2; A.tail[e] = T; }
        return;
    }
    const int cap = A.p.max_tess_points;
    const float2* row = A.outline + (size_t)ent.posture_row * A.p.max_points;
    const int per = (n + VF_TESS_THREADS - 1) / VF_TESS_THREADS;
    const int a = min(tid * per, n), b = min(a + per, n);
    unsigned long long sum = 0;
    for (int j = a; j < b; ++j) {
        const float2 pv = row[j == 0 ? n - 1 : j - 1], pt = row[j];
        float dx, dy;
        sum += (unsigned long long)vf_edge(pv.x, pv.y, pt.x, pt.y, A.p.max_distance, cap, dx, dy) + 1ull;
    }
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (int t = 0; t < VF_TESS_THREADS; ++t) { const unsigned long long v = s_part[t]; s_part[t] = run; run += v; }
        const bool over = run > (unsigned long long)cap;
        A.len[e] = over ? -2 : (int)run;
        A.tail[e] = T;
        if (over) s_part[0] = ~0ull;
    }
    __syncthreads();
    if (s_part[0] == ~0ull) return;                                                     // nothing of an entry that does not fit is written
    unsigned long long at = s_part[tid];
    double2* out = A.tess + (size_t)e * cap;
    const float md = (float)A.p.max_distance;
    for (int j = a; j < b; ++j) {
        const float2 pv = row[j == 0 ? n - 1 : j - 1], pt = row[j];
        float dx, dy;
        const int cnt = vf_edge(pv.x, pv.y, pt.x, pt.y, A.p.max_distance, cap, dx, dy);
        for (int i = 1; i <= cnt; ++i) {                                                // previous + direction * i * max_distance, float32 throughout
            const float fi = (float)i;
            const float qx = pv.x + (dx * fi) * md, qy = pv.y + (dy * fi) * md;
            out[at++] = make_double2((double)qx, (double)qy);
        }
        out[at++] = make_double2((double)pt.x, (double)pt.y);
    }
}

__device__ __forceinline__ double vf_correct(double a) {                               // correct_angle (:67-72); an angle takes one turn at most here
    for (int k = 0; k < 4 && a > VF_PI; ++k) a -= VF_TWO_PI;
    for (int k = 0; k < 4 && a <= -VF_PI; ++k) a += VF_TWO_PI;
    return a;
}
__device__ __forceinline__ double vf_max(double a, double b) { return a < b ? b : a; }   // std::max / std::min as they order their arguments
__device__ __forceinline__ double vf_min(double a, double b) { return b < a ? b : a; }

// the state of one bin: both layers of the five members of VisualField::eye
struct VfBin {
    double dep1, dep2, hd1, hd2;
    float2 p1, p2;
    int id1, id2, fov1, fov2;
};

// plot_projected_line's loop body (:113-148) for one bin
__device__ __forceinline__ void vf_plot(VfBin& s, double d, int id, float2 rp, int fov, double hd, int fish) {
    if (s.dep1 > d) {
        if (s.id1 != fish && s.id1 != id && s.dep2 > s.dep1) { s.dep2 = s.dep1; s.id2 = s.id1; s.p2 = s.p1; s.fov2 = s.fov1; s.hd2 = s.hd1; }
        s.dep1 = d; s.id1 = id; s.p1 = rp; s.fov1 = fov; s.hd1 = hd;
        if (id == fish) { if (s.dep2 != VF_INVALID) s.dep2 = VF_INVALID; }                 // remove 2. stage after self occlusions
    } else if (s.id1 != fish && id != s.id1 && s.dep2 > d) {
        s.dep2 = d; s.id2 = id; s.p2 = rp; s.fov2 = fov; s.hd2 = hd;
    }
}

__global__ __launch_bounds__(VF_THREADS) void k_vf_cast(const VfArgs A) {
    __shared__ double s_d[VF_LDS], s_hd[VF_LDS];
    __shared__ float2 s_rp[VF_LDS];
    __shared__ uint32_t s_se[VF_LDS];                      // start | end << 10 | fov << 20
    __shared__ int32_t s_id[VF_LDS];
    __shared__ uint32_t s_wcnt[2][VF_WAVES];
    if (*A.flag) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, o = blockIdx.x >> 1, eye = blockIdx.x & 1;
    const trexhip_vf_observer* ob = A.observers + o;
    const int f = ob->frame, own = ob->entry, lo = A.frame_entries[f], hi = A.frame_entries[f + 1];
    int over = 0;
    for (int k = lo + tid; k < hi; k += VF_THREADS) over |= A.len[k] == -2;
    over = __syncthreads_or(over);
    const int status = over ? 2 : A.len[own] < 0 ? 1 : 0;
    VfBin s;
    s.dep1 = s.dep2 = VF_INVALID; s.hd1 = s.hd2 = -1.0; s.p1 = s.p2 = make_float2(0.f, 0.f); s.id1 = s.id2 = -1; s.fov1 = s.fov2 = 0;   // eye::eye()
    if (status == 0) {
        const int T_obs = A.tail[own], fish = A.entries[own].id;
        const double ex = ob->eye_x[eye], ey = ob->eye_y[eye], ea = ob->eye_angle[eye], max_d = A.p.max_d;
        const int wlo = wave * 64, whi = wlo + 63;
        int fill = 0, par = 0;
        // every wave walks the waiting records in order and each bin thread applies those that hold its bin
        auto apply = [&]() {
            for (int j0 = 0; j0 < fill; j0 += 64) {
                const int j = j0 + lane;
                const uint32_t se = j < fill ? s_se[j] : 0x3FFu;                     // start 1023: touches nothing
                const int st = (int)(se & 0x3FFu), en = (int)((se >> 10) & 0x3FFu);
                unsigned long long m = __ballot(st <= whi && en >= wlo);
                while (m) {
                    const int jj = j0 + __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t w = s_se[jj];
                    if (tid >= (int)(w & 0x3FFu) && tid <= (int)((w >> 10) & 0x3FFu))
                        vf_plot(s, s_d[jj], s_id[jj], s_rp[jj], (int)(w >> 20), s_hd[jj], fish);
                }
            }
        };
        for (int k = lo; k < hi; ++k) {
            const int n = A.len[k];
            if (n <= 0) continue;                                                    // not used (:552)
            const trexhip_vf_entry ent = A.entries[k];
            const int T = A.tail[k];
            const double posx = (double)ent.pos_x, posy = (double)ent.pos_y;
            double right = (double)((long long)T + 1);                               // :571-572
            double left = (double)(unsigned long long)((long long)n - (long long)T);
            if (left == 0) left = (double)n - right;                                 // :435-436
            if (right == 0) right = (double)n - left;
            const double rx = posx - ex, ry = posy - ey;                             // e.rpos = pos - e.pos
            const double2* P = A.tess + (size_t)k * A.p.max_tess_points;
            for (int base = 0; base < 2 * n; base += VF_CHUNK) {
                if (fill + VF_CHUNK > VF_LDS) {
                    __syncthreads();
                    apply();
                    __syncthreads();
                    fill = 0;
                }
                const int r = base + tid;
                bool keep = false;
                uint32_t se = 0;
                double d = 0, hd = 0;
                float2 rpf = make_float2(0.f, 0.f);
                if (r < 2 * n) {
                    const int i = r >> 1;
                    // the records of point i: (previous, pt) then (ptp, pt), previous = points[n - 1], ptp = points[(n - 2) % n] at i = 0
                    const int i0 = (r & 1) == 0 ? (i == 0 ? n - 1 : i - 1) : (i >= 2 ? i - 2 : i == 1 ? n - 1 : (n >= 2 ? n - 2 : 0));
                    const double2 pt0 = P[i0], pt1 = P[i];
                    hd = 1 - fabs((double)i - (double)T_obs) / ((i > T_obs ? left : right) + 1);
                    hd *= 255;
                    const double l0x = pt0.x + rx, l0y = pt0.y + ry, l1x = pt1.x + rx, l1y = pt1.y + ry;
                    // project_angles_1d (:74-94)
                    double a0 = atan2(l0y, l0x), a1 = atan2(l1y, l1x);
                    a0 = vf_correct(a0); a1 = vf_correct(a1);
                    a0 = a0 - ea; a1 = a1 - ea;
                    a0 = vf_correct(a0); a1 = vf_correct(a1);
                    if (a1 < a0) { const double t = a0; a0 = a1; a1 = t; }
                    const double first = (a0 >= VF_FOV_START && a0 <= VF_FOV_END) ? (a0 - VF_FOV_START) / VF_FOV_LEN * (double)VF_RES : -1;
                    const double second = (a1 >= VF_FOV_START && a1 <= VF_FOV_END) ? (a1 - VF_FOV_START) / VF_FOV_LEN * (double)VF_RES : -1;
                    if (first >= 0 || second >= 0) {
                        const double rpx = (first >= 0 ? pt0.x : pt1.x) + posx, rpy = (first >= 0 ? pt0.y : pt1.y) + posy;
                        d = (rpx - ex) * (rpx - ex) + (rpy - ey) * (rpy - ey);
                        rpf = make_float2((float)rpx, (float)rpy);
                        // plot_projected_line's range (:98-107)
                        double x0 = first, x1 = second;
                        x0 = (x0 == -1.0) ? x1 : vf_max(0.0, x0 - 1.0);
                        x1 = (x1 == -1.0) ? x0 : vf_min((double)VF_RES - 1.0, x1 + 1.0);
                        const uint32_t start = (uint32_t)vf_max(0.0, x0), end = (uint32_t)vf_min((double)VF_RES, ceil(x1));
                        const double v = 1.0 - vf_min(1.0, vf_max(0.0, d / max_d));
                        const uint32_t fov = (uint32_t)(unsigned char)(v * v * 255);
                        keep = start <= end && start < (uint32_t)VF_RES;                // else the loop of :109 has no iteration
                        se = start | end << 10 | fov << 20;
                    }
                }
                const unsigned long long m = __ballot(keep);
                if (lane == 0) s_wcnt[par][wave] = (uint32_t)__popcll(m);
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < VF_WAVES; ++w) { const int c = (int)s_wcnt[par][w]; before += w < wave ? c : 0; total += c; }
                if (keep) {
                    const int at = fill + before + __popcll(m & ((1ull << lane) - 1ull));   // < fill + VF_CHUNK <= VF_LDS
                    s_se[at] = se; s_id[at] = ent.id; s_d[at] = d; s_rp[at] = rpf; s_hd[at] = hd;
                }
                fill += total;
                par ^= 1;
            }
        }
        __syncthreads();
        apply();
    }
    const size_t at1 = ((size_t)blockIdx.x * 2) * VF_RES + tid, at2 = at1 + VF_RES;
    if (A.depth) { A.depth[at1] = s.dep1; A.depth[at2] = s.dep2; }
    if (A.ids) { A.ids[at1] = s.id1; A.ids[at2] = s.id2; }
    if (A.points) { A.points[at1] = s.p1; A.points[at2] = s.p2; }
    if (A.fov) { A.fov[at1] = (uint8_t)s.fov1; A.fov[at2] = (uint8_t)s.fov2; }
    if (A.hd) { A.hd[at1] = s.hd1; A.hd[at2] = s.hd2; }
    if (A.status && tid == 0 && eye == 0) A.status[o] = status;
}

static size_t vf_up16(size_t v) { return (v + 15) / 16 * 16; }

}  // namespace trexhip

using namespace trexhip;

extern "C" {

void trexhip_default_vf_params(trexhip_ctx* ctx, trexhip_vf_params* p) {
    if (!p) return;
    const double w = ctx ? (double)ctx->p.width : 0.0, h = ctx ? (double)ctx->p.height : 0.0;
    p->max_d = w * w + h * h;                  // SQR(Tracker::average().cols) + SQR(Tracker::average().rows), VisualField.cpp:61
    p->max_distance = 5.0;                     // VisualField.h:68
    p->max_points = 512;                       // trexhip_default_posture_params' max_points
    p->max_tess_points = 1024;
}

int trexhip_visual_field_device(trexhip_ctx* ctx, const trexhip_vf_params* vp, const float* d_outline, const trexhip_posture_info* d_posture_info,
                                const int32_t* d_frame_entries, int32_t n_frames, const trexhip_vf_entry* d_entries, int32_t n_entries,
                                const trexhip_vf_observer* d_observers, int32_t n_observers, double* d_depth, int32_t* d_ids, float* d_points,
                                uint8_t* d_fov, double* d_head_distance, int32_t* d_status) {
    const char* who = "trexhip_visual_field_device: ";
    if (!ctx || !vp) { set_error(std::string(who) + "null context or parameters"); return TREXHIP_E_INVALID; }
    if (n_frames < 0 || n_entries < 0 || n_observers < 0) { set_error(std::string(who) + "negative count"); return TREXHIP_E_INVALID; }
    if (vp->max_points < 1 || vp->max_tess_points < vp->max_points || vp->max_tess_points > VF_MAX_TESS) {
        set_error(std::string(who) + "max_points must be >= 1 and max_tess_points in max_points..2^24");
        return TREXHIP_E_INVALID;
    }
    if (n_observers > 0 && (n_frames == 0 || n_entries == 0)) { set_error(std::string(who) + "observers without frames or entries"); return TREXHIP_E_INVALID; }
    if (n_observers == 0) return TREXHIP_OK;
    if (!d_outline || !d_posture_info || !d_frame_entries || !d_entries || !d_observers) {
        set_error(std::string(who) + "outlines, posture info, frame offsets, entries and observers are required");
        return TREXHIP_E_INVALID;
    }
    const size_t o_flag = 0, o_len = 16, o_tail = o_len + vf_up16((size_t)n_entries * 4), o_tess = o_tail + vf_up16((size_t)n_entries * 4),
                 total = o_tess + (size_t)n_entries * (size_t)vp->max_tess_points * sizeof(double2);
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    hipStream_t s = ctx->stream;
    if (int rc = ctx->vf.reserve(ctx, total, "trexhip_visual_field_device")) return rc;     // n_entries x max_tess_points tessellated points
    uint8_t* base = ctx->vf.as<uint8_t>();
    TH_CHECK_HIP(hipMemsetAsync(base + o_flag, 0, 16, s));
    VfArgs A{};
    A.p = *vp;
    A.outline = reinterpret_cast<const float2*>(d_outline); A.info = d_posture_info;
    A.frame_entries = d_frame_entries; A.n_frames = n_frames;
    A.entries = d_entries; A.n_entries = n_entries;
    A.observers = d_observers; A.n_observers = n_observers;
    A.depth = d_depth; A.ids = d_ids; A.points = reinterpret_cast<float2*>(d_points); A.fov = d_fov; A.hd = d_head_distance; A.status = d_status;
    A.flag = reinterpret_cast<uint32_t*>(base + o_flag);
    A.len = reinterpret_cast<int32_t*>(base + o_len);
    A.tail = reinterpret_cast<int32_t*>(base + o_tail);
    A.tess = reinterpret_cast<double2*>(base + o_tess);
    const int m = std::max(n_frames, n_observers);
    hipLaunchKernelGGL(k_vf_check, dim3((m + 255) / 256), dim3(256), 0, s, A);
    hipLaunchKernelGGL(k_vf_tess, dim3(n_entries), dim3(VF_TESS_THREADS), 0, s, A);
    hipLaunchKernelGGL(k_vf_cast, dim3(2u * (unsigned)n_observers), dim3(VF_THREADS), 0, s, A);
    TH_CHECK_HIP(hipGetLastError());
    uint32_t flag = 0;
    TH_CHECK_HIP(hipMemcpyAsync(&flag, base + o_flag, 4, hipMemcpyDeviceToHost, s));
    TH_CHECK_HIP(hipStreamSynchronize(s));
    if (flag) {
        set_error(std::string(who) + "frame offsets do not ascend from 0 within n_entries, or an observer names a frame outside the call or an entry outside "
                                     "its frame; no output was written");
        return TREXHIP_E_INVALID;
    }
    return TREXHIP_OK;
}

}  // extern "C"
