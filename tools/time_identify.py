"""Times trexhip_identify_device on resident crops (dev tool, needs the GPU): per case the device-event time per call and the host's enqueue time
per call, after a warm-up that lets a small chain be captured.  Cases: 100, 1000 and 25600 crops 80x80 and 1000 crops 64x64, 1 channel, FP16X3.
One JSON line; the keys end in _us and carry the graph setting, so that runs with graphs on and off can share one table (tools/ab_time.py).
   python tools/time_identify.py [--graphs 0]"""
import json
import os
import sys
import time

graphs = sys.argv[sys.argv.index("--graphs") + 1] if "--graphs" in sys.argv else "1"
os.environ["TREXHIP_GRAPHS"] = graphs
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from trex_amd import capi, weights

CLASSES = 100
CASES = ((80, 100, 400), (80, 1000, 200), (80, 25600, 20), (64, 1000, 200))       # size, crops, timed calls

out = {"graphs": int(graphs)}
rng = np.random.default_rng(1)
for size, n, calls in CASES:
    seg = capi.Segmenter(capi.default_params(64, 64, max_batch=1))
    seg.load_weights(weights.pack_blob(weights.synthetic_state(CLASSES, 1, 1, size, size), CLASSES, 1, size, size))
    crops = torch.from_numpy(rng.integers(0, 256, (n, size, size, 1), dtype=np.uint8)).cuda()
    probs = torch.empty((n, CLASSES), dtype=torch.float32, device="cuda")
    for _ in range(5):
        seg.identify_device(crops.data_ptr(), n, probs.data_ptr())
    seg.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()                  # the context runs on torch's current stream: the events bracket exactly its calls
    t0 = time.perf_counter()
    for _ in range(calls):
        seg.identify_device(crops.data_ptr(), n, probs.data_ptr())
    host = time.perf_counter() - t0
    ev1.record()
    torch.cuda.synchronize()
    tag = f"{size}x{size}_n{n}_graphs{graphs}"
    out[tag + "_device_us"] = round(ev0.elapsed_time(ev1) * 1e3 / calls, 2)
    out[tag + "_host_us"] = round(host * 1e6 / calls, 2)
    seg.close()
print(json.dumps(out))
