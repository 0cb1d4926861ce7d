// cnn_conv3p.h -- conv3 of the identity network's default chain, walked PAIR BY PAIR (round 5).  Included by cnn.hip after cnn_wpre.h.
//
// Network: visual_identification_network_torch.py:184-258 (V118_3, eval mode): conv3 = 5x5 'same', 64 -> 128 channels on the 20x20 map, then
// ReLU and the 2x2 max-pool.  Arithmetic: F(4,5) Winograd along x -- 8 position products per kernel row give 4 neighbouring outputs --, direct
// along y, both operands as two fp16 pieces, three piece products per term, fp32 accumulation; per position the sums run over the 16-channel
// chunks, then the kernel rows (the order of k_conv5_wino and of the chunk-major kernel of rounds 3-4, k_conv5_wpre, whose position sums are
// bit-identical to these).
//
// What is different from k_conv5_wpre is the ORDER OF THE POSITIONS.  It walked a pass chunk by chunk with all 8 positions of a chunk inside one tap
// group: every position is final only at the very end of the pass, 16 accumulator tuples (all 256 accumulator registers) are live throughout,
// and the output transform A^T, the pool and the stores -- ~1000 vector instructions per pass -- wait behind the last tap with nothing to run
// beside them (one wave per SIMD): 19 % of a pass.  Here a pass is 4 UNITS of 40 taps, one per position pair in the order (1,2) (3,4) (5,6) (0,7),
// each over all 64 input channels (V3 is laid out for that, cnn_wpre.h).  A^T combines exactly these pairs:
//     e_k = M_a + M_b, o_k = M_a - M_b;   y0 = e1 + e2 + e3 + M0,  y1 = o1 + 2 o2 + o3 / 2,  y2 = e1 + 4 e2 + e3 / 4,  y3 = o1 + 8 o2 + o3 / 8 + M7
// so the pair of unit g is folded into the four partial outputs UNDER THE TAPS OF UNIT g + 1 (1-2 vector instructions per MFMA: free, a wave's
// own vector instructions between its MFMAs cost nothing up to ~5 per MFMA, profiles/r05_ubench_simd.txt), and the last unit's pair, the pool,
// bias, ReLU and the stores run under unit 0 of the wave's NEXT pass.  Two accumulator banks (a unit writes one while the other is folded) =
// 128 accumulator registers instead of 256; the partial outputs of both tiles live in 128 vector registers.  Nothing of the epilogue is left
// behind the last tap; the next pass's A offsets are computed under the last unit as well.
// (y0 takes position 0 last instead of first: the only change in the order of a sum against k_conv5_wpre; probabilities differ by <= 6e-7.)
//
// Measured (25600 crops, A/B against k_conv5_wpre on the same boxes): 4.42 -> 4.21, 4.57 -> 4.38 ms; matrix pipe 0.64 ->
// 0.69 busy (profiles/r05_pmc_conv_pair.txt) at a clock that FALLS as the pipe fills (1.56 -> 1.50 GHz: the kernel is power-limited; with its
// operand loads switched off the same 960 MFMAs per pass run at 2.6 GHz).  A first version with the same tap order was SLOWER than
// k_conv5_wpre (4.50 against 4.39): 47 instructions per tap instead of 28 -- spilled scalars, hoisted address arithmetic, lane masks around the
// DMA -- and a wave issues one instruction per ~4.5 cycles, so a tap of 6 MFMAs (192 cycles) has room for ~40.  Weight fragments 3 / 5 / 7 taps
// ahead: 4.52 / 4.39 / 4.39; A fragments 2 taps ahead: no change.

//
// The LISTED form (cnn_skip3.h) computes only the row pairs whose V3 rows hold more than the empty crop's image.  A pass is then SIX listed row
// pairs -- 60 of the 64 tile slots, so that a lane's pair slot and its place in the pair are the same in every pass -- from at most two runs (one
// crop's consecutive pairs): 2 pA + 4 and 2 pB + 4 V3 rows, at most NR together.  k_pair_list (cnn_skip_kernels.h) has written per pass what the
// kernel needs (skip3_describe) and k_act3_fill where each of its rows comes from (skip3_row_words): a crop's own rows from V3, its background
// rows from the empty crop's image, which lies in front of V3 and behind it in V3's allocation -- k_v3_fill copies nothing where this form runs,
// and what V3 holds outside the own rows is never read.  The staging goes through one buffer resource per pass whose base the table names; the
// table's entry i, in lane i, is the byte offset of row slot i's source, and a lane fetches its slot's entry and adds its constant (a shift, a
// ds_bpermute_b32 and an add per DMA instruction, where a compare, a select and an add jumped the gap between the runs before); what lies
// behind the pass's rows has an offset behind the resource's end and reads zeros as before; y comes from the listed pair's q; the stores go to
// the listed pair's place in act3, a per-lane select between two of the pass's six
// pair offsets (tiles i and i + 4 h can lie in different pairs).  Everything else -- the taps, their order, the fold, the tail -- is the dense
// form's, so a listed pair's outputs are the dense kernel's bits.  Both forms are launched; `words` (SK3_USE) names the one that runs.
// Measured (profiles/conv3_listed_pairs.txt; the benchmark's 25600 crops: 31381 listed passes against 40000 dense ones): 4511 -> 3573 us under a
// kernel trace, a listed pass cost 1.01 dense passes.  With the background rows read from the image (profiles/v3_direct_rows.txt, 31393 listed
// passes): 3669 -> 3542 us under a kernel trace, 116.9 -> 112.8 ns per listed pass (half of what it stages now comes from 200 KB that stay in
// L2), 1.00 dense passes; with the table entry fetched in the tap that needs it -- its wait in front of that tap's first MFMA -- 3634 us.  The
// dense instance keeps its registers (256 + 210, no scratch, 2 vector spills), the listed one has 256 + 242, no scratch, no vector spills (256 +
// 230 and 20 spills before).  (The pass's values are plain scalars on purpose: as members of a struct handed to the lambdas they stayed in scratch memory, 104
// bytes per lane in BOTH instances.)
//
// The WINDOWED listed form (L = Skip3XGeom; cnn_skip3.h: skip3_window) computes, of every listed pair of a crop whose blob reaches at most WT3 = 3
// of a row's 5 tiles, only those 3: a pass is TEN pair slots of 6 tiles -- again 60 of the 64 tile slots -- from at most two runs, 28 V3 rows.
// What differs from the full-width listed form is the LDS image (Wino3Pass, cnn_geom.h) and three constants: an LDS row holds the window's 3 tiles of
// each of the 8 position groups (768 bytes of the V3 row's 1280), gathered by the staging -- the lane's constant maps its 16 LDS bytes to the head
// of their 160-byte group of the V3 row and the row's table entry carries t0 * 32 bytes (skip3_row_words), so the staging instructions and the
// tap loop are the same ones, fewer (12 DMA instructions per wave and unit instead of 14) --; the lane's tile is pair slot t / 6, place t % 6; and the
// pair's act3 offset carries the window's 2 t0 pooled columns.  Per output element nothing depends on the slot or window it lands in: the bits are the
// dense kernel's.  The 4 pooled columns outside the window hold the empty crop's bits, written by k_act3_fill.
// Measured (profiles/conv3_windowed.txt; the benchmark's 25600 crops: 7347 windowed + 19658 full-width passes where the row-only list has 31383):
// 116.4 ns per windowed pass against 113.7 ns per full-width pass under a kernel trace, 3423 -> 3091 us for both instances.  Registers: 256 + 236,
// no scratch, no vector spills; the dense and the full-width listed instance keep theirs (256 + 210, 256 + 242).
//
// Passes of TILE SLOTS (L = Skip3TGeom, Skip3TXGeom; cnn_skip3.h): whole pairs leave 4 of the 64 tile slots idle, and both MFMA M-blocks run whole
// either way.  A listed pass is now up to 64 CONSECUTIVE tiles of its list's pair sequence: tile slot t = m * 32 + j is tile o + t of it, o the
// (even) tiles the pass begins into its first pair -- pair slot (o + t) / TPP and place (o + t) % TPP are the pass's, not the lane's for good.  They
// are made where the next pass's A offsets are, under the last unit (a_base): the pair's entry comes out of the descriptor words the wave holds in
// its lanes (raw_w) by one ds_bpermute_b32, and the tile's act3 offset -- its pair's, its place's, the window's, out of the resource's range for
// a slot past the pass's tile count -- is made there once per pass and kept by the lane whose number is the slot; the tail reads the two offsets
// of an accumulator row pair from lanes t0 and t0 + 4, compile-time lane numbers, where it added compile-time places to two of the pass's
// scalars.  The tap loop has the instructions it had.  A full-width pass touches up to 8 pairs: 24 V3 rows, 25 row slots of 1360 bytes per piece
// (133 KB of LDS), 17 staging instructions per wave and unit instead of 14; a windowed one up to 12 pairs: 32 rows, 33 slots of 816 bytes (105 KB),
// 13 instead of 12, and a row table of 64 words, one per lane, where the others have 32 (RW).  One workgroup per CU as before.  Registers: 256 +
// 242 and 256 + 234, no scratch, no vector spills; the dense and the pair-slot instances are unchanged (256 + 210 and 2 spills, 256 + 242, 256 +
// 236).  TREXHIP_CONV_GEOM bit 20 runs the pair-slot instances.
// Measured: profiles/conv3_tile_slots.txt.
template <bool LISTED, class L = Skip3Geom>
__global__ __launch_bounds__(256) void k_conv5_wpair(const uint8_t* __restrict__ v3, const uint4* __restrict__ wp /*[4][5][8][2][2][128] x 16 B*/,
                                                     const float* __restrict__ bias, float* __restrict__ out, const float out_scale,
                                                     const int n_crops, uint32_t* __restrict__ pass_ctr,
                                                     const int n_big_dense /* tickets of PK passes; the passes behind them go out one by one */,
                                                     const int* __restrict__ desc /* LISTED: DESC words per pass */,
                                                     const uint32_t* __restrict__ rowsrc /* LISTED: Skip3Reach::WORDS per pass, the sources of its rows */,
                                                     const uint32_t* __restrict__ words /* Net::d_skip; null: the dense form, unconditionally */) {
    constexpr int CI = 64, CO = 128, S = 20, TPW = 2;
    constexpr int BD = 5;         // taps of lead of the weight fragments (measured above)
    constexpr int AD = 1;         // taps of lead of the A fragments
    constexpr int PK = 4;         // passes per ticket: their halo rows are L2 hits
    constexpr int DT0 = 2;        // the tap at which the DMA of the next unit starts
    using G = WinoGeom<CI, CO, S, TPW>;
    static_assert(G::NTHR == 256 && G::RP0 == 1280 && G::NCH * 2 * G::RP0 == V3_ROWB && G::NT == 4 && G::WM == 1, "geometry");
    static_assert(BD >= 1 && BD <= 7, "weight ring of 8 taps");
    extern __shared__ __attribute__((aligned(16))) uint8_t ldsb[];
    __shared__ int s_next_pass;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    using LR = Skip3Reach;
    using P = Wino3Pass<L::TILES, L::NR>;                 // the LDS image of a pass
    constexpr bool WIN = L::TILES != G::TPR;              // the windowed listed form
    constexpr bool TS = Skip3Tiled<L>::value;             // a listed pass of tile slots
    constexpr int RW = Skip3Tiled<L>::ROW_WORDS;          // words of a pass's row table: its base in the last one
    static_assert(LISTED || (!WIN && !TS), "only a listed pass has a window or tile slots");
    static_assert(LR::ROWB == V3_ROWB && SkipGeom::V3_ROWS == S, "the images in front of V3 and behind it are S rows of V3_ROWB bytes");
    static_assert((WIN || TS || (P::NR == G::NR && P::RP == G::RP && P::BUF == G::BUF)) && (TS || L::SLOTS * P::TPP <= G::MB) && L::PAIRS * 2 == S, "a listed pass fits the dense pass's rows and tiles");
    static_assert(!TS || (P::TPP - 2 + G::MB - 1) / P::TPP < L::SLOTS, "tile slots: every lane's pair slot is one of the descriptor's");
    if (words && (words[SK3_USE] != 0) != LISTED) return;
    const int total_tiles = n_crops * G::TPC;
    const int n_pass = LISTED ? __builtin_amdgcn_readfirstlane((int)words[WIN ? SK3X_RAN : SK3_RAN]) : (total_tiles + G::MB - 1) / G::MB;
    const int n_big = LISTED ? (n_pass >= 16 * (int)gridDim.x ? (int)((long long)n_pass * 7 / 8) / 4 : 0) : n_big_dense;
    const int big_end = n_big * PK;
    auto ticket_first = [&](const int t) { return t < n_big ? t * PK : big_end + (t - n_big); };
    int pass = ticket_first((int)blockIdx.x);
    if (pass >= n_pass) return;
    const uint32_t lds0 = (uint32_t)(uintptr_t)ldsb;
    // Staging of a unit by LDS-DMA (no registers, no LDS store instructions).  The two piece planes of a buffer are ONE linear LDS range from row
    // slot 1 of piece 0 to the last row of piece 1 (piece 1's zero row in between) = NI instructions of 1 KB; lane l of instruction i covers
    // byte o = 1024 i + 16 l of it and fetches its unit of (row, piece) from the unit's rows through a BUFFER resource over exactly the pass's
    // rows: what is out of range -- rows the pass does not have, the lanes over piece 1's zero row, the lanes past the last row (they land on
    // the next buffer's zero row, or in the kilobyte of slack behind the second buffer) -- is given an offset outside the resource and comes
    // back as ZEROS, which is what a zero row holds.  No clamps, no lane masks, no branches: per instruction one scalar add (M0), the lane's
    // precomputed offset, the load.  Wave w issues the instructions w, w + 4, ...: NDW per wave and unit, one per tap.
    constexpr int RNG = (2 * P::NR + 1) * P::RP, NI = (RNG + 1023) / 1024, NDW = (NI + 3) / 4;
    static_assert(DT0 + NDW <= 40 - BD, "the DMA instructions are older than the last 2 BD weight loads of a unit");
    static_assert(NI * 1024 - RNG <= 1024, "slack behind the second buffer");
    uint32_t dvo[NDW];
#pragma unroll
    for (int k = 0; k < NDW; ++k) {
        const int o = (wave + 4 * k) * 1024 + lane * 16;
        const int pc = o >= (P::NR + 1) * P::RP ? 1 : 0, q = o - pc * (P::NR + 1) * P::RP;
        const int row = q / P::RP, w = q - row * P::RP;
        const bool real = q < P::NR * P::RP && o < RNG;
        // (WIN: the LDS row's position group w / PS lies G::PS bytes apart in the V3 row; the window's first tile comes with the row's source)
        const int wv = WIN ? (w / P::PS) * G::PS + w % P::PS : w;
        const uint32_t inrow = (uint32_t)(pc * 1280 + (w < P::RP0 ? wv : G::RP0 - 16 - (WIN ? 2 * LR::TILEB : 0)));
        // LISTED: the row slot and the byte in the row; the slot's source is the pass's (its table's entry NR: none)
        dvo[k] = LISTED ? (real ? (uint32_t)row << LR::ROW_SHIFT | inrow : (uint32_t)P::NR << LR::ROW_SHIFT)
                        : real ? (uint32_t)(row * V3_ROWB) + inrow : 0x80000000u;
    }
    const uint32_t mbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds0 + P::RP + wave * 1024));
    // (LISTED: qmin_ is the row of V3's allocation the pass's resource starts at -- the empty crop's image lies in front of V3 and behind it,
    // cnn_skip3.h --, and the resource has one size: the table's offsets are in range, what it calls none is not)
    auto stage_rsrc = [&](const int g, const int qmin_, const int nrows_) {
        const unsigned long long base = wave_uniform64(reinterpret_cast<unsigned long long>(v3) + (unsigned long long)(long long)(qmin_ - (LISTED ? S : 0)) * V3_ROWB + (unsigned)(g * 2560));
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(base), 0,
                                                 LISTED ? (int)(LR::NUM_RECORDS - (unsigned)(g * 2560)) : __builtin_amdgcn_readfirstlane(nrows_ * V3_ROWB - g * 2560), 0x00020000);
    };
    // (M0 is written and not restored: nothing else in this kernel reads it -- checked in the ISA)
    // (LISTED: the pass's table, entry i in lane i: the lane fetches its row slot's entry -- P3_SRC, a shift and a permute, one tap AHEAD of the
    // instruction that needs it: the permute's answer takes as long as an LDS read, and waiting for it in the tap that issued it holds up that tap's
    // first MFMA -- and adds its constant)
#define P3_SRC(k_, tab_) (uint32_t)__builtin_amdgcn_ds_bpermute((int)(dvo[k_] >> (LR::ROW_SHIFT - 2)), (int)(tab_))
#define P3_DMA(k_, srs_, buf_, src_)                                                                                             \
    do {                                                                                                                         \
        if ((k_) < NDW - 1 || wave + 4 * (NDW - 1) < NI) {                                                                       \
            const uint32_t vo_ = LISTED ? dvo[k_] + (src_) : dvo[k_];                                                            \
            asm volatile("s_add_u32 m0, %0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds"                          \
                         :: "s"(mbase), "n"((buf_) * P::BUF + (k_) * 4096), "v"(vo_), "s"(srs_) : "memory", "scc");               \
        }                                                                                                                        \
    } while (0)
    for (int i = tid; i < 4 * (P::RP / 16); i += G::NTHR) {          // row slot 0 of the four planes = the zero row
        const int pl = i / (P::RP / 16), o = i - pl * (P::RP / 16);
        *reinterpret_cast<uint4*>(ldsb + pl * P::PLANE + o * 16) = make_uint4(0, 0, 0, 0);
    }
    const __amdgpu_buffer_rsrc_t wrs = make_rsrc(wp, (uint32_t)(G::NCH * 40 * G::BV * 16));
    const int boff = (h * CO + wave * 32 + j) * 16;
    const int co = wave * 32 + j;
    const float bz = bias[co];
    const int ooff = (4 * h * CO + co) * 4;
    // LISTED: the lane's two tiles m * 32 + j: pair slot (the idle tiles 60 .. 63 take the last one's rows; their stores are dropped) and place in the pair
    int lps[TPW], lr2[TPW];
#pragma unroll
    for (int m = 0; m < TPW; ++m) {
        const int t = m * 32 + j;
        lps[m] = t / P::TPP < L::SLOTS ? t / P::TPP : L::SLOTS - 1;
        lr2[m] = t % P::TPP;
    }
    // what a pass is: the dense form's rows qmin .. qmin + nrows - 1; LISTED: the descriptor's scalars (rows of run A, gap, the pairs' act3 offsets
    // relative to the pass's first pair) and the lane's two pair entries
    // (the descriptor as it is loaded: word lane % DESC and the lane's two pair entries)
    int raw_w = 0, ent[TPW] = {};
    uint32_t tab = 0;
    auto pass_fetch = [&](const int pass_) {
        const int* d = desc + (size_t)pass_ * L::DESC;
        raw_w = d[lane & (L::DESC - 1)];
        tab = rowsrc[(size_t)pass_ * RW + (lane & (RW - 1))];
        if (TS) return;           // (tile slots: the pair entries come out of raw_w, a_base)
#pragma unroll
        for (int m = 0; m < TPW; ++m) ent[m] = d[S3_SLOT + lps[m]];
    };
    auto pass_decode = [&](int& qmin_, int& gp0_, int& span_, uint32_t (&rel_)[L::SLOTS], int& tiles_) {
        const int w = raw_w;
        qmin_ = __builtin_amdgcn_readlane((int)tab, RW - 1);
        gp0_ = __builtin_amdgcn_readlane(w, S3_GP0);
        span_ = __builtin_amdgcn_readlane(w, S3_SPAN);
        if (TS) { tiles_ = __builtin_amdgcn_readlane(w, S3_TILES); return; }      // (the act3 offsets are the lanes': a_base)
#pragma unroll
        for (int s2 = 0; s2 < L::SLOTS; ++s2) {
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane(w, S3_SLOT + s2), rp = e >> 16;
            // (WIN: the window's first pooled column, 2 t0, goes into the pair's offset: slot and place stay compile-time per accumulator row)
            rel_[s2] = rp == (uint32_t)S3_IDLE ? 0x80000000u
                     : rp * (uint32_t)(G::TPP * CO * 4) + (WIN ? ((e >> S3_T0_SHIFT) & S3_T0_MASK) * (uint32_t)(2 * CO * 4) : 0u);
        }
    };
    int qmin = 0, nrows = 0, gp0 = 0, span = 0, tiles = 0;
    uint32_t rel[L::SLOTS] = {};
    if (LISTED) { pass_fetch(pass); pass_decode(qmin, gp0, span, rel, tiles); }
    else wino_pass_rows<G, S>(pass, total_tiles, qmin, nrows);
    const __amdgpu_buffer_rsrc_t srs0 = stage_rsrc(0, qmin, nrows);
#pragma unroll
    for (int k = 0; k < NDW; ++k) P3_DMA(k, srs0, 0, P3_SRC(k, tab));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // tap tt of unit g: chunk tt / 10, kernel row (tt % 10) / 2, position PAIRS[g][tt & 1]; its weights [chunk][ky][position] x BV x 16 bytes
    auto w_off = [](const int g, const int tt) {
        const int hp = tt & 1, p = g == 3 ? (hp ? 7 : 0) : 2 * g + 1 + hp;
        return ((tt / 10) * 40 + ((tt % 10) / 2) * 8 + p) * G::BV * 16;
    };
    uint4 bq[8][2];
#pragma unroll
    for (int t = 0; t < BD; ++t) {
        bq[t][0] = buf_load16(wrs, boff, w_off(0, t));
        bq[t][1] = buf_load16(wrs, boff, w_off(0, t) + 2 * CO * 16);
    }
    // A-operand byte offsets of this lane's two tiles, per kernel row: the row slot (out-of-crop rows -> the zero row) + the tile's 32 bytes
    // (per tile: the offset of its own input row and of the zero row, and its y; per kernel row a compare and a select)
    // TS: tile slot t = m * 32 + j of a pass is tile o + t of its pair sequence: pair slot (o + t) / TPP, whose entry the wave holds in lane
    // S3_SLOT + slot of raw_w, and place (o + t) % TPP -- per pass, where the pair-slot form has them per lane for good.  The act3 offset of the
    // tile -- its pair's, its place's and the window's; past the pass's tile count, out of the resource's range -- is made here as well, once
    // per pass: toff[m], of which lane l keeps that of tile slot l (otab_n) for the tail to read by lane number
    uint32_t toff[TPW] = {};
    auto a_base = [&](const int pass_, const int qmin_, const int tiles_, const int m, int& inr, int& zr, int& yy) {
        if (TS) {
            constexpr int MUL = P::TPP == 10 ? 205 : 171, SH = P::TPP == 10 ? 11 : 10;      // x / TPP for x < 72
            static_assert(P::TPP == 10 || P::TPP == 6, "the division by multiplication");
            const int o = tiles_ & S3_O_MASK, cnt = tiles_ >> S3_COUNT_SHIFT, t = m * 32 + j;
            const int x = o + t, slot = (x * MUL) >> SH, r2 = x - slot * P::TPP, par = r2 & 1;
            const int e = __builtin_amdgcn_ds_bpermute((S3_SLOT + slot) * 4, raw_w);
            yy = 2 * ((e >> 8) & S3_Q_MASK) + par; zr = (r2 >> 1) * 32 + h * 16; inr = ((e & 0xff) + par) * P::RP + zr;
            const uint32_t rp = (uint32_t)e >> 16;
            toff[m] = t < cnt && rp != (uint32_t)S3_IDLE
                    ? rp * (uint32_t)(G::TPP * CO * 4) + (uint32_t)(r2 * CO * 4) + (WIN ? ((e >> S3_T0_SHIFT) & S3_T0_MASK) * (uint32_t)(2 * CO * 4) : 0u)
                    : 0x80000000u;
            return;
        }
        if (LISTED) {             // (the entries fetched last: this pass's in front of the loop, the next one's under the last unit)
            const int r2 = lr2[m], par = r2 & 1, e = ent[m];
            yy = 2 * ((e >> 8) & (WIN ? S3_Q_MASK : 0xff)) + par; zr = (r2 >> 1) * 32 + h * 16; inr = ((e & 0xff) + par) * P::RP + zr;
            return;
        }
        int T = pass_ * G::MB + m * 32 + j;
        if (T > total_tiles - 1) T = total_tiles - 1;
        const int gp = T / G::TPP, r2 = T - gp * G::TPP;
        const int tx = r2 >> 1, qo = 2 * gp + (r2 & 1);
        yy = qo % S; zr = tx * 32 + h * 16; inr = (qo - qmin_ + 1) * G::RP + zr;
    };
    auto a_offset = [&](const int inr, const int zr, const int yy, const int ky) {
        const int iy = yy + ky - 2;
        return (iy >= 0 && iy < S) ? inr + (ky - 2) * P::RP : zr;
    };
    int aoff[TPW][5];
#pragma unroll
    for (int m = 0; m < TPW; ++m) {
        int inr, zr, yy;
        a_base(pass, qmin, tiles, m, inr, zr, yy);
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) aoff[m][ky] = a_offset(inr, zr, yy, ky);
    }
    int an_in[TPW] = {}, an_z[TPW] = {}, an_y[TPW] = {};
    // TS: the act3 offset of tile slot l in lane l, of this pass and of the pass whose tail is still to run
    uint32_t otab = h ? toff[1] : toff[0], otab_prev = 0x80000000u;
    // two accumulator banks x two tiles x the two positions of a pair; the partial outputs y0..y3 of both tiles.  All of it lives across
    // passes (the tail of a pass runs inside the next one); the first pass's "previous pass" stores into an empty buffer resource (dropped)
    // one accumulator register read where it is written (the compiler's own copies move a whole 16-register tuple to vector registers at
    // the first use: 32 registers the kernel does not have).  The MFMAs that wrote the tuple are a barrier and two taps back.
    auto P3_ACC = [](const float a) { float v; asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a)); return v; };
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 acc[2][TPW][2];
    float y[TPW][4][16];
#pragma unroll
    for (int m = 0; m < TPW; ++m) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc[k >> 1][m][k & 1] = zero16;
#pragma unroll
            for (int r = 0; r < 16; ++r) y[m][k][r] = 0.f;
        }
    }
    // (an empty volatile asm on a result keeps its arithmetic at the tap it is written under: left alone, the compiler sinks all of it to the
    // first use of the value -- the tail, one pass later -- and the registers of three units' accumulators with it)
#define P3_PIN(x_) asm volatile("" : "+v"(x_))
    __amdgpu_buffer_rsrc_t ors_prev = make_rsrc(out, 0);
    uint32_t rel_prev[L::SLOTS] = {};                  // LISTED: the act3 offsets of the pairs of the pass whose tail is still to run
    // pool (rows r, r + 1 x outputs 0,1 / 2,3), bias, ReLU, store.  Accumulator rows r, r + 1 (r even) of lane half h are the tiles i, i + 1 = the
    // two rows of a row pair at one tx, and the tile number of the even one IS the pooled output's index: T = 10 gp + 2 tx (TPP = 10 is even, so
    // T & 1 = the row's parity).  No division: the address is the lane's constant offset + a compile-time one, and tiles past the end of the
    // batch fall outside the pass's buffer resource (dropped by the hardware).
    auto tail = [&](const __amdgpu_buffer_rsrc_t rs, const int m, const int rr) {
        const int r = 2 * rr, i = (r & 3) + 8 * (r >> 2);
        const float a0 = y[m][0][r] + P3_ACC(acc[1][m][0][r]), a1 = y[m][0][r + 1] + P3_ACC(acc[1][m][0][r + 1]);
        const float d0 = y[m][3][r] + P3_ACC(acc[1][m][1][r]), d1 = y[m][3][r + 1] + P3_ACC(acc[1][m][1][r + 1]);
        const float v0 = fmaxf(fmaxf(a0, y[m][1][r]), fmaxf(a1, y[m][1][r + 1]));
        const float v1 = fmaxf(fmaxf(y[m][2][r], d0), fmaxf(y[m][2][r + 1], d1));
        if (TS) {
            // tile slots t0 = m * 32 + i (h = 0) and t0 + 4 (h = 1): their offsets are those lanes' of the pass's table
            const int t0 = m * 32 + i;
            const uint32_t o0 = (uint32_t)__builtin_amdgcn_readlane((int)otab_prev, t0), o1 = (uint32_t)__builtin_amdgcn_readlane((int)otab_prev, t0 + 4);
            const int vo = co * 4 + (int)(h ? o1 : o0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(v0 * out_scale + bz, 0.f)), rs, vo, 0, 2 /* nt */);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(v1 * out_scale + bz, 0.f)), rs, vo + CO * 4, 0, 2);
            return;
        }
        if (LISTED) {
            // tiles t0 = m * 32 + i (h = 0) and t0 + 4 (h = 1): pair slot and place in the pair are compile-time, the pair's offset is the pass's
            // (all of it in the lane's offset: that is what the resource's range check looks at)
            const int t0 = m * 32 + i, t1 = t0 + 4;
            const uint32_t o0 = rel_prev[t0 / P::TPP] + (uint32_t)((t0 % P::TPP) * CO * 4);
            const uint32_t o1 = t1 / P::TPP < L::SLOTS ? rel_prev[t1 / P::TPP < L::SLOTS ? t1 / P::TPP : 0] + (uint32_t)((t1 % P::TPP) * CO * 4) : 0x80000000u;
            const int vo = co * 4 + (int)(h ? o1 : o0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(v0 * out_scale + bz, 0.f)), rs, vo, 0, 2 /* nt */);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(v1 * out_scale + bz, 0.f)), rs, vo + CO * 4, 0, 2);
            return;
        }
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(v0 * out_scale + bz, 0.f)), rs, ooff, (m * 32 + i) * CO * 4, 2 /* nt */);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(v1 * out_scale + bz, 0.f)), rs, ooff, (m * 32 + i + 1) * CO * 4, 2);
    };
    // the pair of unit g (bank g & 1) folded into the partial outputs, one accumulator row of one tile at a time
    auto fold = [&](const int g, const int m, const int r) {
        const float a = P3_ACC(acc[g & 1][m][0][r]), b = P3_ACC(acc[g & 1][m][1][r]);
        const float e = a + b, o = a - b;
        if (g == 0) { y[m][2][r] = e; y[m][1][r] = o; P3_PIN(y[m][2][r]); P3_PIN(y[m][1][r]); }
        if (g == 1) {
            const float e1 = y[m][2][r], o1 = y[m][1][r];
            y[m][0][r] = e1 + e; y[m][1][r] = o1 + 2.f * o; y[m][2][r] = e1 + 4.f * e; y[m][3][r] = o1 + 8.f * o;
        }
        if (g == 2) { y[m][0][r] += e; y[m][1][r] += 0.5f * o; y[m][2][r] += 0.25f * e; y[m][3][r] += 0.125f * o; }
        if (g >= 1) { P3_PIN(y[m][0][r]); P3_PIN(y[m][1][r]); P3_PIN(y[m][2][r]); P3_PIN(y[m][3][r]); }
    };
    for (;;) {
        const int tleft = total_tiles - pass * G::MB;
        const __amdgpu_buffer_rsrc_t ors = LISTED ? make_rsrc(out + (size_t)gp0 * (G::TPP * CO), (uint32_t)(span * (G::TPP * CO * 4)))
                                                  : make_rsrc(out + (size_t)(pass * G::MB) * CO, (uint32_t)((tleft < G::MB ? tleft : G::MB) * CO * 4));
        int next_pass = pass + 1;
        const bool draw = pass >= big_end || pass % PK == PK - 1;          // the last pass of a ticket draws the next one
        if (draw && tid == 0) s_next_pass = ticket_first((int)atomicAdd(pass_ctr, 1u) + (int)gridDim.x);   // read by everyone after the first unit's barrier
        bool have_next = false;
        int qmin_n = qmin, nrows_n = nrows, gp0_n = gp0, span_n = span, tiles_n = tiles;
        uint32_t otab_n = otab;
        uint32_t rel_n[L::SLOTS];
#pragma unroll
        for (int s2 = 0; s2 < L::SLOTS; ++s2) rel_n[s2] = rel[s2];
#pragma clang loop unroll(full)
        for (int g = 0; g < 4; ++g) {
            const bool last_u = g == 3;
            if (!LISTED && last_u) {
                if (draw) next_pass = s_next_pass;
                have_next = next_pass < n_pass;
                if (have_next) wino_pass_rows<G, S>(next_pass, total_tiles, qmin_n, nrows_n);
            }
            // (without a next pass the descriptor fetched is this pass's own: the next = this one once more)
            if (LISTED && last_u) pass_decode(qmin_n, gp0_n, span_n, rel_n, tiles_n);
            const uint8_t* pbase = ldsb + (g & 1) * P::BUF;
            // staged under this unit: the next unit of this pass, or unit 0 of the next pass (without one: this pass's once more, into the buffer
            // nobody reads again)
            const int sg = last_u ? 0 : g + 1;
            const int sqmin = last_u ? qmin_n : qmin, snrows = last_u ? nrows_n : nrows;
            const __amdgpu_buffer_rsrc_t srs = stage_rsrc(sg, sqmin, snrows);
            uint32_t src_next = 0;
            // A fragments AD taps ahead (tap tt: position slot (tt / 10) * 2 + (tt & 1), kernel row (tt % 10) / 2)
            uint4 af[AD + 1][TPW][2];
#pragma unroll
            for (int a = 0; a < AD; ++a)
#pragma unroll
                for (int m = 0; m < TPW; ++m) {
                    af[a][m][0] = *reinterpret_cast<const uint4*>(pbase + (a & 1) * P::PS + aoff[m][a / 2]);
                    af[a][m][1] = *reinterpret_cast<const uint4*>(pbase + (a & 1) * P::PS + aoff[m][a / 2] + P::PLANE);
                }
#pragma clang loop unroll(full)
            for (int tt = 0; tt < 40; ++tt) {
                const int cur = tt % (AD + 1), nxt = (tt + AD) % (AD + 1);
                // (LISTED: the source of the next tap's DMA instruction, asked for in front of this tap's MFMAs; under the last unit `tab` is the
                // next pass's already: fetched under the unit before)
                const uint32_t src_cur = src_next;
                if (LISTED && tt + 1 >= DT0 && tt + 1 < DT0 + NDW) src_next = P3_SRC(tt + 1 - DT0, tab);
                if (tt + AD < 40) {
                    const uint8_t* an = pbase + (((tt + AD) / 10) * 2 + ((tt + AD) & 1)) * P::PS;
#pragma unroll
                    for (int m = 0; m < TPW; ++m) {
                        af[nxt][m][0] = *reinterpret_cast<const uint4*>(an + aoff[m][((tt + AD) % 10) / 2]);
                        af[nxt][m][1] = *reinterpret_cast<const uint4*>(an + aoff[m][((tt + AD) % 10) / 2] + P::PLANE);
                    }
                }
                const int wt = tt + BD < 40 ? w_off(g, tt + BD) : w_off(sg, tt + BD - 40);
                bq[(tt + BD) % 8][0] = buf_load16(wrs, boff, wt);
                bq[(tt + BD) % 8][1] = buf_load16(wrs, boff, wt + 2 * CO * 16);
                // LISTED: the next pass's descriptor is fetched late in the unit before the last -- the ticket is there behind the first unit's
                // barrier -- and taken apart at the top of the last one, whose staging needs its scalars
                if (LISTED && g == 2 && tt == 34) {
                    if (draw) next_pass = s_next_pass;
                    have_next = next_pass < n_pass;
                    pass_fetch(have_next ? next_pass : pass);
                }
                if (tt >= DT0 && tt < DT0 + NDW) P3_DMA(tt - DT0, srs, (g & 1) ^ 1, src_cur);
                const int hp = tt & 1;
                const f16x8 b1 = __builtin_bit_cast(f16x8, bq[tt % 8][0]);
                const f16x8 b2 = __builtin_bit_cast(f16x8, bq[tt % 8][1]);
                f16x8 a1[TPW], a2[TPW];
#pragma unroll
                for (int m = 0; m < TPW; ++m) { a1[m] = __builtin_bit_cast(f16x8, af[cur][m][0]); a2[m] = __builtin_bit_cast(f16x8, af[cur][m][1]); }
#pragma unroll
                for (int m = 0; m < TPW; ++m) acc[g & 1][m][hp] = mfma16(a2[m], b1, tt < 2 ? zero16 : acc[g & 1][m][hp]);
#pragma unroll
                for (int m = 0; m < TPW; ++m) acc[g & 1][m][hp] = mfma16(a1[m], b2, acc[g & 1][m][hp]);
#pragma unroll
                for (int m = 0; m < TPW; ++m) acc[g & 1][m][hp] = mfma16(a1[m], b1, acc[g & 1][m][hp]);
                if (g == 0) {
                    // the previous pass's tail (its positions 0 and 7 are in bank 1, which this pass first writes in unit 1)
                    if (tt >= 2 && tt < 34 && !(tt & 1)) tail(ors_prev, (tt - 2) / 16, ((tt - 2) / 2) % 8);
                } else if (tt >= 2 && tt < 34) {
                    fold(g - 1, (tt - 2) / 16, (tt - 2) % 16);
                }
                // the next pass's A offsets, in place: kernel row ky was last read for tap 31 + 2 ky of this unit, one tap ahead
                if (last_u && have_next && (tt == 28 || tt == 30)) a_base(next_pass, qmin_n, tiles_n, (tt - 28) / 2, an_in[(tt - 28) / 2], an_z[(tt - 28) / 2], an_y[(tt - 28) / 2]);
                if (TS && last_u && have_next && tt == 31) otab_n = h ? toff[1] : toff[0];
                if (last_u && have_next && (tt == 39 || (tt >= 32 && tt < 39 && !(tt & 1)))) {
                    const int ky = tt == 39 ? 4 : (tt - 32) / 2;
#pragma unroll
                    for (int m = 0; m < TPW; ++m) aoff[m][ky] = a_offset(an_in[m], an_z[m], an_y[m], ky);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 2 * TPW, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 10, 0);
#pragma unroll
                for (int k = 0; k < 3 * TPW; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x246, 8, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // this wave's part of the next unit has landed: loads return in order, so everything older than the 2 x BD weight fragments in
            // flight is complete -- the DMA instructions were issued before them (stores in between only make the wait stricter)
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * BD) : "memory");
            __syncthreads();
        }
        ors_prev = ors;
        otab_prev = otab; otab = otab_n;
#pragma unroll
        for (int s2 = 0; s2 < L::SLOTS; ++s2) { rel_prev[s2] = rel[s2]; rel[s2] = rel_n[s2]; }
        if (!have_next) break;
        pass = next_pass; qmin = qmin_n; nrows = nrows_n; gp0 = gp0_n; span = span_n; tiles = tiles_n;
    }
    // the last pass's tail has no next pass to run under (fold of unit 2 ran under unit 3; unit 3's pair is positions 0 and 7, taken by the tail itself)
#pragma unroll
    for (int b = 0; b < 16; ++b) tail(ors_prev, b / 8, b % 8);
#undef P3_DMA
#undef P3_SRC
#undef P3_PIN
}
