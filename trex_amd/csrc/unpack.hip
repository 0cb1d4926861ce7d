// unpack.hip -- pv::Frame::read_from for the frames of a stored batch, on the device: the inverse of pack.hip.
//
// Given the V_6 frame bodies of a batch in HBM (layout and every bounds rule: pv_read.h) the context ends up holding what it holds behind
// trexhip_segment_device: frame table, blob records, lines, pixels, the pooled totals -- and a frame image with every blob's stored pixels
// painted at its lines, because the track-stage kernels read grey values from ctx->d_frames at the (y, x) of a blob's lines, not from
// the pixel arrays.  The re-threshold pass additionally walks the detect pass's raster tables (lines of a frame sorted by (y, x0), a row
// index and a line -> blob map); they are rebuilt here from the loaded lines.
//
//   k_load_index    one wave per frame walks the only serial chain (a blob's byte length is 4 + 4 m + its pixels): 64 lanes load and
//                   validate a blob's lines at once, the pixel count is reduced in the wave; no workgroup barrier.  Leaves per blob
//                   {byte offset, lines, pixels, start_y, line / pixel offset in the frame} and per frame {counts, flag}
//   k_load_scan     exclusive scan of the three counts over the frames (frame order: the pooled layout does not depend on timing),
//                   frame table, pooled totals
//   k_load_decode   one wave per blob: eol prefix count -> y, lines, pixel copy + paint (8 bytes per step, tails byte by byte), the sums /
//                   box / min-max / bid of k_gather restated on exact integers; counts the lines of every image row
//   k_load_rows, k_load_scatter, k_load_rank    the raster tables: row index, lines bucketed by row, then placed by their rank in the row
// Bound: the bodies are read twice (index: line bytes only), 8 bytes per line + 2 bytes per pixel + the blob records are written: a few
// tens of MB for 256 frames of 100 individuals -- the chain walk's latency, not bandwidth, sets the time.
#include "internal.h"
#include "pv_read.h"

namespace trexhip {

struct LoadBlob { uint32_t off, n_lines, n_pixels, start_y, run_begin, pix_begin; };
struct LoadFrame { uint32_t n_blobs, n_lines, n_pixels, flags; };

__device__ __forceinline__ uint32_t lw_sum32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t lw_min32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}
__device__ __forceinline__ uint32_t lw_max32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}
__device__ __forceinline__ uint64_t lw_sum64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ uint32_t lw_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, d);
        if (lane >= (uint32_t)d) v += u;
    }
    return v;
}

// ---- the chain: one wave per frame ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_load_index(const uint8_t* __restrict__ bodies, const unsigned long long* __restrict__ offsets,
                                                   const uint32_t W, const uint32_t H, const uint32_t cap_blobs, const uint32_t cap_runs,
                                                   const uint32_t cap_pixels, LoadBlob* __restrict__ index, LoadFrame* __restrict__ meta,
                                                   unsigned long long* __restrict__ timestamps) {
    const uint32_t f = blockIdx.x, lane = threadIdx.x;
    const unsigned long long o0 = offsets[f], o1 = offsets[f + 1];
    const uint64_t len = o1 >= o0 ? o1 - o0 : 0ull;                  // every read below stays in front of body + len
    const uint8_t* body = bodies + o0;
    bool good = pvr::frame_head_ok(body, len);
    const uint32_t n = good ? pvr::frame_blobs(body) : 0u;
    if (timestamps && lane == 0) timestamps[f] = good ? pvr::frame_timestamp(body) : 0ull;
    uint32_t nl = 0;
    uint64_t np = 0, o = pvr::FRAME_HEAD;
    for (uint32_t b = 0; good && b < n; ++b) {
        pvr::BlobHead h;
        if (!pvr::read_blob_head(body, len, o, h)) { good = false; break; }
        const uint8_t* lp = body + o + pvr::BLOB_HEAD;
        uint32_t y_base = h.start_y, carry_x1 = 0, carry_eol = 1, px = 0;
        for (uint32_t j0 = 0; j0 < h.mask_size; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool act = j < h.mask_size;
            pvr::Line l = {0u, 0u, 0u};
            if (act) l = pvr::read_line(lp + (size_t)pvr::LINE_BYTES * j);
            const unsigned long long eolm = __ballot(act && l.eol);
            const uint32_t y = y_base + (uint32_t)__popcll(eolm & ((1ull << lane) - 1ull));
            uint32_t prev_x1 = (uint32_t)__shfl_up((int)l.x1, 1), prev_eol = (uint32_t)__shfl_up((int)l.eol, 1);
            if (lane == 0) { prev_x1 = carry_x1; prev_eol = carry_eol; }
            const bool ok = !act || pvr::line_ok(l, y, prev_eol != 0u, prev_x1, W, H);
            if (__ballot(!ok)) { good = false; break; }
            px += lw_sum32(act ? pvr::line_pixels(l) : 0u);           // <= 65535 lines of <= 32768 pixels: fits 32 bits
            y_base += (uint32_t)__popcll(eolm);
            carry_x1 = (uint32_t)__shfl((int)l.x1, 63); carry_eol = (uint32_t)__shfl((int)l.eol, 63);
        }
        if (!good) break;
        const uint64_t op = o + pvr::BLOB_HEAD + (uint64_t)pvr::LINE_BYTES * h.mask_size;
        if (!pvr::pixels_fit(op, px, len)) { good = false; break; }
        if (lane == 0 && b < cap_blobs) {
            LoadBlob ib;
            ib.off = (uint32_t)o; ib.n_lines = h.mask_size; ib.n_pixels = px; ib.start_y = h.start_y; ib.run_begin = nl; ib.pix_begin = (uint32_t)np;
            index[(size_t)f * cap_blobs + b] = ib;
        }
        nl += h.mask_size; np += px; o = op + px;                     // np <= len < 2^32
    }
    if (good && !pvr::frame_end_ok(o, len)) good = false;
    if (lane == 0) {
        LoadFrame m;
        m.n_blobs = good ? n : 0u; m.n_lines = good ? nl : 0u; m.n_pixels = good ? (uint32_t)np : 0u;
        m.flags = !good ? TREXHIP_FRAME_MALFORMED
                        : ((nl > cap_runs ? TREXHIP_FRAME_OVERFLOW_RUNS : 0u) | ((n > cap_blobs || np > cap_pixels) ? TREXHIP_FRAME_OVERFLOW_OUTPUT : 0u));
        meta[f] = m;
    }
}

// ---- frame table: exclusive scan over the frames (one workgroup: batches are a few hundred frames) --------------------------------------
__global__ __launch_bounds__(256) void k_load_scan(const LoadFrame* __restrict__ meta, const int n, trexhip_frame_info* __restrict__ info,
                                                   uint32_t* __restrict__ totals) {
    __shared__ LoadFrame s_m[256];
    __shared__ uint32_t s_begin[256][3];
    __shared__ uint32_t s_run[3];
    if (threadIdx.x < 3) s_run[threadIdx.x] = 0u;
    __syncthreads();
    for (int f0 = 0; f0 < n; f0 += 256) {
        const int f = f0 + (int)threadIdx.x;
        LoadFrame m = {0u, 0u, 0u, 0u};
        if (f < n) m = meta[f];
        s_m[threadIdx.x] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t rb = s_run[0], rr = s_run[1], rp = s_run[2];
            for (int k = 0; k < 256 && f0 + k < n; ++k) {
                s_begin[k][0] = rb; s_begin[k][1] = rr; s_begin[k][2] = rp;
                if (s_m[k].flags == 0u) { rb += s_m[k].n_blobs; rr += s_m[k].n_lines; rp += s_m[k].n_pixels; }   // a flagged frame reserves nothing
            }
            s_run[0] = rb; s_run[1] = rr; s_run[2] = rp;
        }
        __syncthreads();
        if (f < n) {
            trexhip_frame_info fi = {};
            const bool kept = m.flags == 0u;
            fi.n_blobs = kept ? m.n_blobs : 0u; fi.n_runs = kept ? m.n_lines : 0u; fi.n_pixels = kept ? m.n_pixels : 0u;
            fi.blob_begin = s_begin[threadIdx.x][0]; fi.run_begin = s_begin[threadIdx.x][1]; fi.pix_begin = s_begin[threadIdx.x][2];
            fi.n_raw_runs = m.n_lines; fi.n_raw_blobs = m.n_blobs;
            fi.flags = m.flags;
            info[f] = fi;
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) totals[threadIdx.x] = s_run[threadIdx.x];
    if (threadIdx.x == 3) totals[3] = 0u;
}

// ---- one wave per blob -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_load_decode(const uint8_t* __restrict__ bodies, const unsigned long long* __restrict__ offsets,
                                                     const uint32_t W, const uint32_t H, const uint32_t cap_blobs, const uint32_t R,
                                                     const LoadBlob* __restrict__ index, const trexhip_frame_info* __restrict__ info,
                                                     trexhip_blob* __restrict__ blobs, uint32_t* __restrict__ blob_frame,
                                                     trexhip_run* __restrict__ runs, uint8_t* __restrict__ pixels, uint8_t* __restrict__ image,
                                                     uint32_t* __restrict__ row_cnt, uint32_t* __restrict__ root_ord, int32_t* __restrict__ blob_map) {
    const uint32_t f = blockIdx.y, lane = threadIdx.x & 63u;
    const trexhip_frame_info fi = info[f];
    if (fi.flags) return;                                             // keeps no blob, paints nothing
    const uint8_t* body = bodies + offsets[f];
    uint8_t* img = image + (size_t)f * H * W;
    for (uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6); k < fi.n_blobs; k += gridDim.x * 4u) {
        const LoadBlob ib = index[(size_t)f * cap_blobs + k];
        const uint8_t* lp = body + ib.off + pvr::BLOB_HEAD;
        const uint8_t* src = lp + (size_t)pvr::LINE_BYTES * ib.n_lines;         // the blob's pixel bytes: ib.n_pixels of them, inside the frame (index pass)
        trexhip_run* rr = runs + fi.run_begin + ib.run_begin;
        uint8_t* px = pixels + fi.pix_begin + ib.pix_begin;
        uint64_t m10 = 0, m01 = 0, m20 = 0, m11 = 0, m02 = 0, sp = 0, spx = 0, spy = 0;
        uint32_t bx0 = 0xffffu, bx1 = 0u, by1 = 0u, pmin = 255u, pmax = 0u, po = 0u, y_base = ib.start_y;
        pvr::Line first = {0u, 0u, 0u};
        for (uint32_t j0 = 0; j0 < ib.n_lines; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool act = j < ib.n_lines;
            pvr::Line l = {0u, 0u, 0u};
            if (act) l = pvr::read_line(lp + (size_t)pvr::LINE_BYTES * j);
            if (j0 == 0) { first.x0 = (uint32_t)__shfl((int)l.x0, 0); first.x1 = (uint32_t)__shfl((int)l.x1, 0); }
            const unsigned long long eolm = __ballot(act && l.eol);
            const uint32_t y = y_base + (uint32_t)__popcll(eolm & ((1ull << lane) - 1ull));
            y_base += (uint32_t)__popcll(eolm);
            const uint32_t L = act ? pvr::line_pixels(l) : 0u;
            const uint32_t incl = lw_incl_scan(L, lane);
            uint32_t off = po + incl - L;
            po += (uint32_t)__shfl((int)incl, 63);
            // (the index pass checked all of this on the same bytes; the test keeps a write inside the image and the tables even if they changed since)
            if (act && l.x0 <= l.x1 && l.x1 < W && y < H && off + L <= ib.n_pixels) {
                trexhip_run q; q.x0 = (uint16_t)l.x0; q.x1 = (uint16_t)l.x1; q.y = (uint16_t)y; q.pad = 0;
                rr[j] = q;
                atomicAdd(row_cnt + (size_t)f * H + y, 1u);
                bx0 = min(bx0, l.x0); bx1 = max(bx1, l.x1); by1 = max(by1, y);
                uint8_t* dst = img + (size_t)y * W + l.x0;
                uint64_t rp = 0;                                      // sum of the line's grey values
                for (uint32_t x = 0; x < L; x += 8u, off += 8u) {
                    const uint32_t rem = min(8u, L - x);
                    unsigned long long w = 0;
                    if (rem == 8u) {                                  // 8 bytes per step; a line's tail byte by byte (no read past the line, no write past it)
                        __builtin_memcpy(&w, src + off, 8);
                        __builtin_memcpy(px + off, &w, 8);
                        __builtin_memcpy(dst + x, &w, 8);
                    } else {
                        for (uint32_t t = 0; t < rem; ++t) {
                            const uint8_t p = src[off + t];
                            px[off + t] = p; dst[x + t] = p;
                            w |= (unsigned long long)p << (8u * t);
                        }
                    }
                    uint32_t s8 = 0, k8 = 0;                          // sum p, sum t * p of the step
#pragma unroll
                    for (uint32_t t = 0; t < 8u; ++t) {
                        if (t < rem) {
                            const uint32_t p = (uint32_t)(w >> (8u * t)) & 0xffu;
                            s8 += p; k8 += t * p;
                            pmin = min(pmin, p); pmax = max(pmax, p);
                        }
                    }
                    rp += s8;
                    spx += (uint64_t)(l.x0 + x) * s8 + k8;
                }
                // sums over x of the line in closed form: exact integers, so the same values as a pixel loop
                const uint64_t L64 = L, xa = l.x0, y64 = y;
                const uint64_t tri = (L64 - 1u) * L64 / 2u;                                  // 0 + 1 + .. + (L - 1)
                const uint64_t sx = xa * L64 + tri;
                m10 += sx;
                m20 += L64 * xa * xa + 2u * xa * tri + (L64 - 1u) * L64 * (2u * L64 - 1u) / 6u;   // sum (xa + t)^2
                m01 += y64 * L64; m02 += y64 * y64 * L64; m11 += y64 * sx;
                sp += rp; spy += rp * y64;
            }
        }
        m10 = lw_sum64(m10); m01 = lw_sum64(m01); m20 = lw_sum64(m20); m11 = lw_sum64(m11); m02 = lw_sum64(m02);
        sp = lw_sum64(sp); spx = lw_sum64(spx); spy = lw_sum64(spy);
        bx0 = lw_min32(bx0); bx1 = lw_max32(bx1); by1 = lw_max32(by1); pmin = lw_min32(pmin); pmax = lw_max32(pmax);
        if (lane == 0) {
            trexhip_blob B = {};
            B.run_begin = ib.run_begin; B.n_runs = ib.n_lines; B.pix_begin = ib.pix_begin; B.n_pixels = ib.n_pixels;     // frame-relative: the ABI's form
            B.x0 = (uint16_t)bx0; B.y0 = (uint16_t)ib.start_y; B.x1 = (uint16_t)bx1; B.y1 = (uint16_t)by1;
            B.bid = pvr::bid_of(first.x0, first.x1, ib.start_y, ib.n_lines);
            B.px_min_max = pmin | (pmax << 8);
            B.parent = 0xffffffffu; B.flags = 0u;
            B.m10 = m10; B.m01 = m01; B.m20 = m20; B.m11 = m11; B.m02 = m02; B.sp = sp; B.spx = spx; B.spy = spy;
            blobs[fi.blob_begin + k] = B;
            blob_frame[fi.blob_begin + k] = f;
            // line -> blob map of the re-threshold pass (blob_map[root_ord[label]]): the label of a loaded line is its blob's index in the frame
            root_ord[(size_t)f * R + k] = k;
            blob_map[(size_t)f * R + k] = (int32_t)k;
        }
    }
}

// ---- raster tables of the re-threshold pass ----------------------------------------------------------------------------------------------
// row_base[y] = lines of the frame in rows above y (exclusive scan of the counts k_load_decode left); the counts are zeroed: k_load_scatter's cursors
__global__ __launch_bounds__(256) void k_load_rows(const uint32_t H, const trexhip_frame_info* __restrict__ info, uint32_t* __restrict__ row_cnt,
                                                   uint32_t* __restrict__ row_base) {
    __shared__ uint32_t s_scan[256];
    __shared__ uint32_t s_run;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    uint32_t* cnt = row_cnt + (size_t)f * H;
    uint32_t* rb = row_base + (size_t)f * (H + 1);
    const bool kept = info[f].flags == 0u;
    if (tid == 0) s_run = 0u;
    __syncthreads();
    for (uint32_t y0 = 0; y0 < H; y0 += 256) {
        const uint32_t y = y0 + tid;
        const uint32_t v = (kept && y < H) ? cnt[y] : 0u;
        s_scan[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {
            const uint32_t u = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += u;
            __syncthreads();
        }
        const uint32_t base = s_run;
        if (y < H) { rb[y] = base + s_scan[tid] - v; cnt[y] = 0u; }
        __syncthreads();
        if (tid == 255) s_run = base + s_scan[255];
        __syncthreads();
    }
    if (tid == 0) rb[H] = s_run;
}

// every line into the bucket of its row, in any order: {x0 | x1 << 16} and {y | blob << 16} (max_blobs <= 65535)
__global__ __launch_bounds__(256) void k_load_scatter(const uint32_t H, const uint32_t R, const trexhip_frame_info* __restrict__ info,
                                                      const trexhip_blob* __restrict__ blobs, const trexhip_run* __restrict__ runs,
                                                      const uint32_t* __restrict__ row_base, uint32_t* __restrict__ row_cur,
                                                      uint32_t* __restrict__ tmp_x, uint32_t* __restrict__ tmp_yk) {
    const uint32_t f = blockIdx.y, lane = threadIdx.x & 63u;
    const trexhip_frame_info fi = info[f];
    if (fi.flags) return;
    const uint32_t* rb = row_base + (size_t)f * (H + 1);
    for (uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6); k < fi.n_blobs; k += gridDim.x * 4u) {
        const uint32_t run_begin = blobs[fi.blob_begin + k].run_begin, n_runs = blobs[fi.blob_begin + k].n_runs;
        for (uint32_t j = lane; j < n_runs; j += 64) {
            const trexhip_run q = runs[fi.run_begin + run_begin + j];
            if (q.y >= H) continue;
            const uint32_t pos = rb[q.y] + atomicAdd(row_cur + (size_t)f * H + q.y, 1u);
            if (pos >= fi.n_runs) continue;                           // cannot happen: the rows were counted from the same lines
            tmp_x[(size_t)f * R + pos] = (uint32_t)q.x0 | ((uint32_t)q.x1 << 16);
            tmp_yk[(size_t)f * R + pos] = (uint32_t)q.y | (k << 16);
        }
    }
}

// a line's place in its row = the lines of the bucket in front of it by (x0, blob, slot): the raster order of the detect pass
__global__ __launch_bounds__(256) void k_load_rank(const uint32_t H, const uint32_t R, const trexhip_frame_info* __restrict__ info,
                                                   const uint32_t* __restrict__ row_base, const uint32_t* __restrict__ tmp_x,
                                                   const uint32_t* __restrict__ tmp_yk, trexhip_run* __restrict__ raster, uint32_t* __restrict__ label) {
    const uint32_t f = blockIdx.y, p = blockIdx.x * 256u + threadIdx.x;
    const trexhip_frame_info fi = info[f];
    if (fi.flags || p >= fi.n_runs) return;
    const size_t fo = (size_t)f * R;
    const uint32_t a = tmp_x[fo + p], b = tmp_yk[fo + p];
    const uint32_t y = b & 0xffffu, k = b >> 16;
    const uint32_t* rb = row_base + (size_t)f * (H + 1);
    const uint32_t s0 = rb[y], s1 = min(rb[y + 1], fi.n_runs);
    const uint32_t key = ((a & 0xffffu) << 16) | k;
    uint32_t rank = 0;
    for (uint32_t j = s0; j < s1; ++j) {
        const uint32_t kj = ((tmp_x[fo + j] & 0xffffu) << 16) | (tmp_yk[fo + j] >> 16);
        rank += (kj < key || (kj == key && j < p)) ? 1u : 0u;
    }
    if (s0 + rank >= fi.n_runs) return;
    trexhip_run q; q.x0 = (uint16_t)(a & 0xffffu); q.x1 = (uint16_t)(a >> 16); q.y = (uint16_t)y; q.pad = 0;
    raster[fo + s0 + rank] = q;
    label[fo + s0 + rank] = k;
}

}  // namespace trexhip

using namespace trexhip;

extern "C" int trexhip_load_frames_v6_device(trexhip_ctx* ctx, const uint8_t* d_bodies, const uint64_t* d_offsets, int32_t n_frames,
                                             uint64_t* d_timestamps) {
    if (!ctx || !d_bodies || !d_offsets) { set_error("trexhip_load_frames_v6_device: null argument"); return TREXHIP_E_INVALID; }
    if (n_frames < 1 || n_frames > ctx->p.max_batch) { set_error("trexhip_load_frames_v6_device: n_frames outside 1..max_batch"); return TREXHIP_E_INVALID; }
    if (ctx->p.pixel_encoding != TREXHIP_ENC_GRAY) { set_error("trexhip_load_frames_v6_device: the V_6 layout holds one byte per pixel (gray); colour encodings came with V_12"); return TREXHIP_E_UNSUPPORTED; }
    if (ctx->p.width > 32768) { set_error("trexhip_load_frames_v6_device: LegacyShortHorizontalLine holds x1 < 32768 (pv.h:36)"); return TREXHIP_E_UNSUPPORTED; }
    if (ctx->p.max_blobs > 65535) { set_error("trexhip_load_frames_v6_device: a frame holds at most 65535 objects (u16 n, pv.cpp:686)"); return TREXHIP_E_UNSUPPORTED; }
    TH_CHECK_HIP(hipSetDevice(ctx->p.device));
    if (int rc = fetch_wait(ctx)) return rc;             // the tables this call overwrites may still be on their way to the host
    const size_t B = (size_t)ctx->p.max_batch, W = (size_t)ctx->p.width, H = (size_t)ctx->p.height, NB = (size_t)ctx->p.max_blobs;
    if (int rc = ensure_staging(ctx, "trexhip_load_frames_v6_device")) return rc;
    if (int rc = ctx->load.reserve(ctx, B * NB * sizeof(LoadBlob) + B * sizeof(LoadFrame), "trexhip_load_frames_v6_device")) return rc;
    LoadBlob* index = ctx->load.as<LoadBlob>();
    LoadFrame* meta = reinterpret_cast<LoadFrame*>(index + B * NB);
    const int n = n_frames;
    const uint32_t w = (uint32_t)W, h = (uint32_t)H, R = (uint32_t)ctx->p.max_runs;
    hipStream_t s = ctx->stream;
    const unsigned long long* offs = reinterpret_cast<const unsigned long long*>(d_offsets);
    uint32_t* totals = ctx->tables.d_totals;
    TH_CHECK_HIP(hipMemsetAsync(ctx->label.d_row_cnt, 0, sizeof(uint32_t) * (size_t)n * H, s));
    hipLaunchKernelGGL(k_load_index, dim3(n), dim3(64), 0, s, d_bodies, offs, w, h, (uint32_t)NB, R, (uint32_t)ctx->p.max_pixels, index, meta,
                       reinterpret_cast<unsigned long long*>(d_timestamps));
    hipLaunchKernelGGL(k_load_scan, dim3(1), dim3(256), 0, s, meta, n, ctx->tables.d_info, totals);
    // four blobs per workgroup; a frame of a few blobs does not need workgroups that find nothing to do
    const unsigned gx_blobs = (unsigned)((NB + 3) / 4 < 64 ? (NB + 3) / 4 : 64);
    hipLaunchKernelGGL(k_load_decode, dim3(gx_blobs, n), dim3(256), 0, s, d_bodies, offs, w, h, (uint32_t)NB, R, index, ctx->tables.d_info, ctx->tables.d_blobs,
                       ctx->tables.d_blob_frame, ctx->tables.d_runs, ctx->tables.d_pixels, ctx->d_staging, ctx->label.d_row_cnt, ctx->label.d_root_ord, ctx->label.d_blob_map);
    hipLaunchKernelGGL(k_load_rows, dim3(n), dim3(256), 0, s, h, ctx->tables.d_info, ctx->label.d_row_cnt, ctx->label.d_row_base);
    hipLaunchKernelGGL(k_load_scatter, dim3(gx_blobs, n), dim3(256), 0, s, h, R, ctx->tables.d_info, ctx->tables.d_blobs, ctx->tables.d_runs, ctx->label.d_row_base, ctx->label.d_row_cnt,
                       ctx->label.d_cur_run, ctx->label.d_pix_begin);
    hipLaunchKernelGGL(k_load_rank, dim3((R + 255u) / 256u, n), dim3(256), 0, s, h, R, ctx->tables.d_info, ctx->label.d_row_base, ctx->label.d_cur_run, ctx->label.d_pix_begin,
                       ctx->label.d_raster, ctx->label.d_parent);
    TH_CHECK_HIP(hipGetLastError());
    // the context as it stands behind launch_segment
    ctx->d_frames = ctx->d_staging;
    ctx->d_color_src = nullptr; ctx->color_ch = 0;
    ctx->batch_invert = 0;                       // stored pixels are what the tracker sees: the segmenter stored 255 - p under image_invert
    ctx->batch_zero_bg = ctx->cfg.zero_bg;
    ctx->tables.valid_n = n;
    ctx->tables.fetched = false;
    ctx->pass2.tables.valid_n = 0;
    ctx->pass2.tables.fetched = false;
    return TREXHIP_OK;
}
