"""The device side of the split-search tests: detect a batch, search every blob's threshold, re-threshold every blob at its own; shared by
tests/test_split_gpu.py and tests/test_split_edges_gpu.py."""
import numpy as np
import torch
from trex_amd import capi

SENTINEL = -7                                                # what the threshold array holds where the search wrote nothing


def device_search(frames, bg, presumed_of, method=1, ranges=(), detect_threshold=15, detect_kw=None, n_search=None, **kw):
    """-> detect tables, presumed_nr, thresholds, split infos, sub-blob tables.  presumed_of(frame result) -> that frame's presumed_nr values;
    n_search: search only the first n_search blobs of the pool (default: all); kw: trexhip_split_params fields"""
    n, H, W = frames.shape
    dkw = dict(threshold=detect_threshold)
    dkw.update(detect_kw or {})
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=n, max_blobs=4096, **dkw))
    seg.set_background(bg)
    d = torch.from_numpy(frames).cuda()
    seg.segment_device(d.data_ptr(), n)
    det = seg.fetch()
    nb = sum(len(r.blobs) for r in det)
    presumed = np.zeros(nb, np.int32)                        # pooled order: frame f's blobs start at info["blob_begin"]
    for r in det:
        presumed[r.info["blob_begin"]:r.info["blob_begin"] + len(r.blobs)] = presumed_of(r)
    d_pres = torch.from_numpy(presumed).cuda()
    d_thr = torch.full((max(nb, 1),), SENTINEL, dtype=torch.int32, device="cuda")
    d_info = torch.zeros(max(nb, 1) * capi.SPLIT_INFO_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    seg.split_search_device(d_pres.data_ptr(), nb if n_search is None else n_search, d_thr.data_ptr(), d_info.data_ptr(), method=method,
                            size_ranges=ranges, **kw)
    if n_search is not None:                                 # the entries past the prefix are no thresholds
        thr = d_thr.cpu().numpy()[:nb]
        info = d_info.cpu().numpy().view(capi.SPLIT_INFO_DTYPE)[:nb]
        seg.close()
        return det, presumed, thr, info, None
    seg.rethreshold_per_blob(d_thr.data_ptr(), method, ranges)
    sub = seg.fetch(rethreshold=True)
    thr = d_thr.cpu().numpy()[:nb]
    info = d_info.cpu().numpy().view(capi.SPLIT_INFO_DTYPE)[:nb]
    seg.close()
    return det, presumed, thr, info, sub
