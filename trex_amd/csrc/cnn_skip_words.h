// cnn_skip_words.h -- the words of Net::d_skip, one table: what the list kernels (cnn_skip_kernels.h) leave for k_conv12_rs, k_conv5_wpair
// (cnn_conv3p.h), k_fc1_split and k_head to read on the device, and for the trexhip_identify_*_stats calls to read back.  No device code.
#pragma once
#include "cnn_skip3.h"

namespace trexhip {

enum : int {
    // the empty crop's images (made at load) and the pass list of conv1+conv2 (cnn_skip.h)
    SK_EMPTY_RANGE = 0,      // the fp16 range flag of the run that made the empty crop's V3 image: non-zero -> every pass is listed
    SK_EMPTY_CTR = 1,        // that run's pass counter
    SK_LEN = 2,              // aligned passes the row rule lists for the last call: the full-width list's length where no crop has a window
    SK_NPASS = 3,            // passes of the last call's batch
    SK_FILLED = 4,           // V3 rows outside those passes: taken from the empty crop's image instead of being computed (copied by k_v3_fill or read in place)
    // the windowed listed conv3 (cnn_skip3.h: skip3_window); all zero where no crop can have a window of conv3 tiles
    SK3X_CROPS = 5,          // crops of the last call whose listed pairs went into windowed passes
    SK3X_PASSES = 6,         // windowed listed passes of the last call: the length of the windowed instance's list
    SK3X_CTR = 7,            // the windowed instance's ticket counter (zeroed by k_pair_list)
    // the listed conv3 and the listed fc1 (cnn_skip3.h)
    SK3_PAIRS = 8,           // row pairs of the last call's batch
    SK3_LISTED = 9,          // row pairs listed
    SK3_PASSES = 10,         // listed full-width passes (all listed passes, where no crop can have a window)
    SK3_FILLED = 11,         // act3 row pairs filled from the empty crop's
    SK3_USE = 12,            // non-zero: the listed form of k_conv5_wpair runs, zero: the dense one
    SK3_EMPTY_CTR = 13,      // the pass counter of the run that made the empty crop's act3
    SK3_FC1E_RANGE = 14,     // the fp16 range flag of the run that made the empty crop's fc1 planes (Net::fc1e): non-zero -> SK_EMPTY_RANGE is raised
    SK3_FC1_LEN = 16,        // .. + PAIRS - 1: crops listed for plane q of the listed fc1 by the last call that listed (skip3_fc1_listed)
    SK3_LAST = SK3_FC1_LEN + Skip3Geom::PAIRS - 1,
    // the windowed conv1+conv2 (cnn_skipx.h); written only by a call whose crops can have windows
    SKX_CROPS = 26,          // crops of the last call that took windowed passes
    SKX_PASSES = 27,         // windowed passes listed by the last call: the length of the windowed instance's list
    SKX_FULL = 28,           // full-width passes listed by the last call (for the crops without a window): the length of the full-width instance's list
    SKX_CTR = 29,            // the windowed instance's ticket counter (zeroed by k_pass_list)
    SKX_V2_READ = 30,        // V2 rows the last call's windowed passes read as new rows, a crop's passes counted as one run (cnn_skipx.h: skipx_v2_rows)
    SKX_V2_MADE = 31,        // ... and how many of them the producers made: the others are background rows.  Both 0 where background rows are made
    // what the listed instances of k_conv5_wpair walk (cnn_skip3.h): passes of tile slots, or -- TREXHIP_CONV_GEOM bit 20 -- the passes of pair slots
    // that SK3_PASSES and SK3X_PASSES count either way (the counters of the stats calls, and what the choice of SK3_USE is made on)
    SK3_RAN = 32,            // the length of the full-width listed instance's list
    SK3X_RAN = 33,           // the length of the windowed listed instance's list
    SK_WORDS = 34
};
static_assert(SK_FILLED < SK3X_CROPS && SK3X_CTR < SK3_PAIRS && SK3_LAST < SKX_CROPS && SKX_V2_MADE < SK3_RAN && SK3X_RAN < SK_WORDS, "no word twice, the last one inside the table");

}  // namespace trexhip
