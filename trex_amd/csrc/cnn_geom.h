// cnn_geom.h -- the geometry of the identity network's kernels that their launches are sized by: pure constexpr, no device code and no HIP, so
// that the kernels (conv_f32.h, cnn.hip, cnn_wpre.h, cnn_any.hip) and the host's launch plan (cnn_plan.h, testable on the CPU) read the same numbers.
// What each layout means is told at the kernel that uses it.
#pragma once
#include <initializer_list>

namespace trexhip {

// k_conv5 (conv_f32.h): exact fp32, full-width bands of ROWS output rows, CIC input channels per staged chunk
template <int CI, int CO, int S, int ROWS, int CIC>
struct ConvGeom {
    static constexpr int PW = S + 4, PH = ROWS + 4;
    static constexpr int STR = CIC + 1;                               // odd pixel stride: conflict-free b32 reads
    static constexpr int RP0 = PW * STR;
    static constexpr int RP = RP0 + ((16 - (RP0 % 32)) + 32) % 32;    // row pitch == 16 (mod 32): rows y, y+1 use disjoint banks
    static constexpr int PATCH = PH * RP;                             // floats
    static constexpr int BT = CIC * CO;                               // floats per weight tile
    static constexpr int NPIX = ROWS * S;
    static constexpr int MT = (NPIX + 31) / 32;
    static constexpr int NT = CO / 32;
    static constexpr int WM = 8 / NT;                                 // wave groups along M
    static constexpr int TPW = (MT + WM - 1) / WM;                    // M tiles per wave
    static constexpr int LDS_BYTES = (PATCH + 2 * BT) * 4;
    static constexpr int BPC = S / ROWS;                              // blocks per crop
};

// k_conv5_split (cnn.hip): the bf16 split, NP pieces per operand
template <int CI, int CO, int S, int ROWS, int NP, int CICP = 16>
struct ConvGeomB {
    static constexpr int CIC = CICP;                                  // input channels per staged chunk (16 or 32)
    static constexpr int PW = S + 4, PH = ROWS + 4;
    static constexpr int PSTRIDE = CIC * 2 + 16;                      // bytes per pixel (data + 16 pad: odd multiple of 16)
    static constexpr int PATCH = PH * PW * PSTRIDE;                   // bytes per piece
    static constexpr int BT = NP * (CIC / 8) * CO * 16;               // bytes per weight tile (NP pieces x CIC/8 k-octets)
    static constexpr int NPIX = ROWS * S;
    static constexpr int MT = (NPIX + 31) / 32;
    static constexpr int NT = CO / 32;
    static constexpr int WM = 8 / NT;
    static constexpr int TPW = (MT + WM - 1) / WM;
    static constexpr int LDS_BYTES = NP * PATCH + 2 * BT;
    static constexpr int BPC = S / ROWS;
};
// the bf16 split: three pieces per operand; NTERMS 6 (a3b1 a2b2 a1b3 a2b1 a1b2 a1b1) or 3 (the last three)
static constexpr int SPLIT_NP = 3;

// k_conv5_stream (cnn.hip): the fp16 two-piece convolution on fp32 activations
template <int CI, int CO, int S, int ROWS, int WAVES>
struct ConvGeomS {
    static constexpr int CIC = 16;
    static constexpr int PW = S + 4, PH = ROWS + 4;
    static constexpr int PSTRIDE = 48;                                  // 16 fp16 + 16 B pad per pixel
    static constexpr int RP0 = PW * PSTRIDE;
    static constexpr int PADU = ((8 - (RP0 / 16) % 16) + 16) % 16;
    static constexpr int RP = RP0 + PADU * 16;                          // row pitch, bytes
    static constexpr int PATCH = PH * RP;                               // bytes per piece
    static constexpr int NCH = CI / CIC;
    static constexpr int NBUF = NCH > 1 ? 2 : 1;
    static constexpr int LDS_BYTES = NBUF * 2 * PATCH;
    static constexpr int NTHR = WAVES * 64;
    static constexpr int NPIX = ROWS * S;
    static constexpr int MT = (NPIX + 31) / 32;
    static constexpr int NT = CO / 32;
    static constexpr int WM = WAVES / NT;
    static constexpr int TPW = (MT + WM - 1) / WM;
    static constexpr int BPC = S / ROWS;
    static constexpr int BV = 2 * 2 * CO;                               // uint4 per tap tile: pieces x k-octets x co
    static constexpr int NQ = PH * PW * 4;                              // float4 per staged chunk
    static constexpr int NITEMS = (NQ + NTHR - 1) / NTHR;
};

// k_conv5_wino (cnn.hip) and k_conv5_wpair (cnn_conv3p.h): Winograd F(4,5) along x, tiles numbered through the whole batch
template <int CI, int CO, int S, int TPW>
struct WinoGeom {
    static constexpr int CIC = 16, NCH = CI / CIC;
    static constexpr int TPR = S / 4, TPP = 2 * TPR, TPC = S * TPR;     // tiles per row / row pair / crop
    static constexpr int NT = CO / 32, WM = NT >= 4 ? 1 : 4 / NT, WAVES = NT * WM, NTHR = WAVES * 64;
    static constexpr int MB = WM * TPW * 32;                            // tiles per pass
    static constexpr int MAXPAIRS = (MB + TPP - 2) / TPP + 1;
    static constexpr int NR = 2 * MAXPAIRS + 4;                         // real input rows a pass can need
    static constexpr int PS = TPR * 32;                                 // bytes per position of a row: tiles x 16 halves
    static constexpr int RP0 = 8 * PS;
    // row pitch: == 5 (mod 8) 16-byte slots when a row pair holds 10 tiles, so that the 16 lanes of a ds_read_b128 lane group
    // (tiles i, i+1 = rows y, y+1 of one column, then the next column) fall into 16 different slots
    static constexpr int RP = RP0 + (((5 - (RP0 / 16) % 8) + 8) % 8) * 16;
    static constexpr int PLANE = (NR + 1) * RP;                         // one piece; slot 0 = the zero row
    static constexpr int BUF = 2 * PLANE;
    static constexpr int LDS_BYTES = 2 * BUF;
    static constexpr int BV = 2 * 2 * CO;                               // uint4 per (ky, position): pieces x k-octets x co
    static constexpr int IPR = TPR * 8;                                 // staging items per row: tile x channel pair
    static constexpr int NQ = NR * IPR;
    static constexpr int NITEMS = (NQ + NTHR - 1) / NTHR;
    static_assert(S % 4 == 0 && CO % 32 == 0 && CI % 16 == 0, "geometry");
    static_assert(NITEMS * 8 <= 40, "staging slices do not fit between the 40 taps");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// k_conv5_wpair's LDS image of a pass (cnn_conv3p.h): NR row slots (and the zero row) of TPR tiles per piece, two pieces, two buffers.  The
// dense form and the full-width listed form hold whole rows (TPR 5: WinoGeom's numbers); the windowed listed form holds the WT3 = 3 tiles of a
// crop's window (cnn_skip3.h), gathered from the V3 row by the staging.
// Row pitch: a ds_read_b128 is served in lane groups of 16 ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of each half wave), and a group is free of
// conflicts when its lanes fall into 16 different 16-byte slots of the 256-byte bank row.  Lane j of a half reads tile j (or 32 + j) = pair slot
// j / (2 TPR), row j & 1 of the pair, tile (j % (2 TPR)) >> 1 of the row, at (row slot * RP + 32 tile) bytes.  Counted over the four groups of both
// of a wave's tiles, for consecutive pairs and for two runs a halo apart, every pitch leaves at least one group with two lanes on one slot; the
// pitches == 5 (mod 8) slots at TPR 5 and == 3 (mod 8) slots at TPR 3 leave exactly one such group, every other pitch 2 to 7 times as many
// conflicts.  (TPR 5: the pitch WinoGeom::RP derived from contiguous lane groups -- the same number.)
template <int TPR_, int NR_>
struct Wino3Pass {
    static_assert(TPR_ == 5 || TPR_ == 3, "pitches counted for 5 and 3 tiles per row");
    static constexpr int TPR = TPR_, TPP = 2 * TPR, NR = NR_;
    static constexpr int PS = TPR * 32, RP0 = 8 * PS;                   // bytes per position of a row; bytes of a row
    static constexpr int PITCH_MOD8 = TPR == 5 ? 5 : 3;
    static constexpr int RP = RP0 + (((PITCH_MOD8 - (RP0 / 16) % 8) + 8) % 8) * 16;
    static constexpr int PLANE = (NR + 1) * RP, BUF = 2 * PLANE, LDS_BYTES = 2 * BUF;
    static_assert(LDS_BYTES + 1024 <= 160 * 1024, "LDS");
};
static_assert(Wino3Pass<5, 20>::RP == WinoGeom<64, 128, 20, 2>::RP && Wino3Pass<5, 20>::LDS_BYTES == WinoGeom<64, 128, 20, 2>::LDS_BYTES &&
              Wino3Pass<5, 20>::PS == WinoGeom<64, 128, 20, 2>::PS, "the full-width pass is WinoGeom's");
static_assert(Wino3Pass<3, 28>::RP == 816, "768 bytes of tiles + 3 slots");

// k_conv2_wpre2 (cnn_wpre.h) and the fused conv1+conv2 kernels on top of it: a pass = RPP row pairs of conv2's output
struct W2bGeom {
    static constexpr int CO = 64, S = 40, TPP = 20, RPP = 3, NR = 2 * RPP + 4;
    // conv1 and conv2 alike: KH x KH 'same' convolution, then a POOL x POOL max-pool.  The fused kernels' row arithmetic (a V2 row reads
    // POOL + KH - 1 crop rows from POOL y - KH / 2 on; a tap row ky reads V2 row y + ky - KH / 2) and the row-skipping rule (cnn_skip.h) use these
    static constexpr int KH = 5, POOL = 2;
    static_assert(NR == POOL * RPP + KH - 1, "the V2 rows a pass reads");
    static constexpr int ROWL = 1280;                                   // one (row, piece, group): 4 positions x 10 tiles x 32 B, in V2 and in LDS
    static constexpr int PLANE = (NR + 1) * ROWL, BUF = 2 * PLANE;      // slot 0 = the zero row; BUF = the two pieces of one position group
    static constexpr int PBUF_OFF = 2 * BUF, PBUF = RPP * 20 * 64 * 4;
    static constexpr int LDS_BYTES = PBUF_OFF + PBUF;
    static constexpr int BV = 2 * 2 * CO;
    static_assert(2 * (LDS_BYTES + 64) <= 160 * 1024, "two workgroups per CU");
};

// the tiled convolutions (conv_tiled.h) of the any-size chain (cnn_any.hip) and of the other identity networks (cnn_arch.hip)
constexpr int C1T = 16;                      // first layer: 16 x 16 windows of 2 x 2 conv pixels per workgroup, one window per thread
constexpr int AW = 64;                       // every further layer: windows per tile = 8 M-tiles of 32 conv pixels
// the tile shape (TX windows wide, 64 / TX high) with the fewest tiles over Ho x Wo windows (the pooled output where the layer pools); 8 x 8 on a tie
struct AnyTiles { int TX, tx_n, tiles; };
inline AnyTiles any_tiles(const int Ho, const int Wo) {
    AnyTiles best{8, (Wo + 7) / 8, ((Ho + 7) / 8) * ((Wo + 7) / 8)};
    for (const int tx : {4, 16}) {
        const int ty = AW / tx, txn = (Wo + tx - 1) / tx, t = ((Ho + ty - 1) / ty) * txn;
        if (t < best.tiles) best = {tx, txn, t};
    }
    return best;
}

static constexpr int FC1_KSPLIT = 10;     // 12800 = 10 x 1280: 500 workgroups at 6400 crops (5: 129 us, 10: 92 us, 20: 102 us + slower head); partial planes summed in k_head
static constexpr int HEAD_CPW = 4;        // crops per wave of k_head
static constexpr int FB_MAX = 1024;       // the range guard's plan lists at most this many crops: more flagged ones and every crop is re-run

// the guard words of a network (Net::d_ovf), in 32-bit words: the fp16 range flag, the pass counters of the persistent conv3 / conv2 (the
// kernels index these three as overflow[0..2]), and the re-run plan of k_guard_plan: count, mode, list
enum : int { OVF_RANGE = 0, OVF_PASS3 = 1, OVF_PASS2 = 2, OVF_PLAN = 4, OVF_WORDS = OVF_PLAN + 2 + FB_MAX };

}  // namespace trexhip
