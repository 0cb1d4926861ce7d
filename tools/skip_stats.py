"""How much of conv1+conv2 the benchmark's crops need (dev tool, needs the GPU): one step of bench.py's default workload (config C4, 256 frames,
gray, FP16X3) through the same Pipeline, then the device counters of the last identify call of lane 0 (trexhip_identify_skip_stats): passes of
the batch, passes the role-split kernel computed, bytes of V3 rows taken from the empty crop's image instead (`v3_bytes_filled`: copied into V3
where the dense conv3 runs; where the listed conv3 runs, as on these crops, nothing is copied and the kernel reads those rows from the image
itself -- the count is the same) -- and the crops' own row statistics, on the host -- and the counters of the listed conv3 (trexhip_identify_skip3_stats): row pairs of the batch, row pairs listed, the passes its listed
form walked (0: the dense kernel ran) against the dense kernel's, bytes of act3 filled from the empty crop's -- and those of the listed fc1
(trexhip_identify_fc1_stats): crop-plane rows of the batch and the rows it computed -- and those of the windowed conv1+conv2
(trexhip_identify_skipx_stats): crops that took windowed passes, those passes, the full-width passes the other crops took (the first counters
keep counting by the row rule alone) -- and (trexhip_identify_bgrow_stats) the rows of conv1's pooled output those passes read against the rows
the kernel made of them, the others being background rows -- and those of the windowed listed conv3 (trexhip_identify_skip3x_stats): crops whose
listed pairs went into windowed passes of 3 tiles, those passes, the full-width listed passes of the other crops (conv3_listed_passes keeps
counting by the row rule alone; conv3_passes_run counts passes of whole pairs, six full-width or ten windowed) -- and the passes the two listed
instances walked (trexhip_identify_skip3_ran: conv3_windowed_passes_ran, conv3_full_width_passes_ran -- the full-width ones are passes of up
to 64 consecutive tiles unless TREXHIP_CONV_GEOM bit 20 is set).  Nothing here is timed.  One JSON line.
   python tools/skip_stats.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from trex_amd import synth, weights
from trex_amd.pipeline import Pipeline

W, H, n_ind, _ = synth.CONFIGS["C4"]
B, classes = 256, 100
frames, bg = synth.batch_torch("C4", B, torch.device("cuda:0"), t0=0)
blob = weights.pack_blob(weights.synthetic_state(classes, 4242), classes)
pipe = Pipeline(W, H, n_ind, B, classes, bg, blob)
n = pipe.run(1, frames.data_ptr())
torch.cuda.synchronize()
lane = pipe.lanes[0]
passes, listed, filled = lane.seg.skip_stats()
pairs3, listed3, passes3, filled3 = lane.seg.skip3_stats()
fc1_rows, fc1_listed = lane.seg.fc1_stats()          # crop-plane rows of the listed fc1 and the rows it computed (0, 0: the dense fc1 ran)
x_crops, x_passes, x_full = lane.seg.skipx_stats()
x3_crops, x3_passes, x3_full = lane.seg.skip3x_stats()
ran_windowed, ran_full = lane.seg.skip3_ran()
v2_read, v2_made = lane.seg.bgrow_stats()            # rows of conv1's pooled output the windowed passes read, and those of them made (0, 0: all are)
crops = lane.crops[:passes * 3 // 20]
rows = (crops != 0).any(dim=2)                       # [n][80]: the row holds a non-zero byte
print(json.dumps({"blobs_per_step": int(n), "crops": int(crops.shape[0]), "passes": passes, "passes_listed": listed,
                  "fraction_listed": round(listed / max(passes, 1), 4), "v3_bytes_filled": filled, "v3_bytes": int(crops.shape[0]) * 20 * 10240,
                  "mean_nonzero_rows_per_crop": round(float(rows.sum(1).float().mean()), 2),
                  "empty_crops": int((~rows.any(1)).sum()),
                  "conv3_pairs": pairs3, "conv3_pairs_listed": listed3, "conv3_fraction_listed": round(listed3 / max(pairs3, 1), 4),
                  "conv3_listed_passes": passes3, "conv3_dense_passes": (pairs3 * 10 + 63) // 64,
                  "conv3_pass_ratio": round(passes3 / max((pairs3 * 10 + 63) // 64, 1), 4), "act3_bytes_filled": filled3,
                  "conv3_passes_run": x3_passes + x3_full, "conv3_run_ratio": round((x3_passes + x3_full) / max((pairs3 * 10 + 63) // 64, 1), 4),
                  "conv3_crops_windowed": x3_crops, "conv3_windowed_passes": x3_passes, "conv3_full_width_passes": x3_full,
                  "conv3_windowed_passes_ran": ran_windowed, "conv3_full_width_passes_ran": ran_full,
                  "conv3_ran_ratio": round((ran_windowed + ran_full) / max(x3_passes + x3_full, 1), 4),
                  "fc1_rows": fc1_rows, "fc1_rows_listed": fc1_listed, "fc1_fraction_listed": round(fc1_listed / max(fc1_rows, 1), 4),
                  "crops_windowed": x_crops, "windowed_passes": x_passes, "full_width_passes": x_full,
                  "windowed_passes_per_crop": round(x_passes / max(x_crops, 1), 3),
                  "v2_rows_read": v2_read, "v2_rows_made": v2_made, "v2_fraction_made": round(v2_made / max(v2_read, 1), 4)}))
pipe.close()
