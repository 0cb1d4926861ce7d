"""trexhip_split_search_device on the constructed cases of tests/split_edge_cases.py: every size-class boundary, the sub-line capacities, size
comparisons one ulp to either side of an edge at non-unit cm_per_pixel, every setting the search reads, and the value extremes.  Every searched blob
equals oracle.split_search in all it reports, and the per-blob re-threshold at the found thresholds equals oracle.threshold_blob line by line."""
import numpy as np
import pytest
from oracle import oracle
from rethreshold_checks import assert_per_blob_equal
from split_device import SENTINEL, device_search
import split_edge_cases as sc

pytestmark = pytest.mark.gpu

FIELDS = ("threshold", "effective_threshold", "initial_action", "n_result", "min_pixel", "max_pixel", "first_size", "min_size_bound")


def search(case, n_search=None):
    """-> device_search's results and, by pooled blob index, the blob's Blob of the table (None in a random scene).  The frames of a batch are
    pooled in the order they finish, which differs from call to call: a blob is known by its frame and its bounding box, never by its index"""
    specs, frame_no = {}, iter(range(len(case.frames)))

    def presumed_of(r):
        f, k0 = next(frame_no), int(r.info["blob_begin"])
        if case.blobs is None:
            specs.update((k0 + j, None) for j in range(len(r.blobs)))
            return np.full(len(r.blobs), case.presumed_all)
        by_origin = {b.origin: b for b in case.blobs if b.frame == f}
        mine = [by_origin[(int(b["x0"]), int(b["y0"]))] for b in r.blobs]
        assert len(mine) == len(by_origin)
        specs.update((k0 + j, b) for j, b in enumerate(mine))
        return np.array([b.presumed for b in mine], np.int32)

    out = device_search(case.frames, case.bg, presumed_of, case.method, list(case.ranges), detect_kw=dict(cm_per_pixel=case.cm, **case.detect_kw),
                        n_search=n_search, algorithm=case.algorithm, **case.split_kw)
    return out, specs


def assert_blob_equals_oracle(case, sp, r, b, spec, pn, got, thr):
    """one pooled blob's split info and threshold against the oracle's search of the same lines and pixels"""
    if pn <= 0:
        assert got["status"] == 3
    elif spec is not None and spec.outcome == "capacity":
        assert got["status"] == 2
    else:
        assert got["status"] == 0
        runs = r.runs[b["run_begin"]:b["run_begin"] + b["n_runs"]]
        px = r.pixels[b["pix_begin"]:b["pix_begin"] + b["n_pixels"]]
        want = oracle.split_search(runs, px, case.bg, case.method, sp, pn, case.connectivity)
        for name in FIELDS:
            assert got[name] == getattr(want, name), (name, got[name], getattr(want, name))
        assert thr == want.effective_threshold
        if spec is not None:
            assert want.threshold == spec.threshold           # the hand-derived one
        return want.threshold >= 0
    assert (got["threshold"], got["effective_threshold"], thr, got["n_result"]) == (-1, -1, -1, 0)
    return False


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_equals_oracle(name):
    case = sc.table()[name]
    (det, presumed, thr, info, sub), specs = search(case)
    sp = oracle.split_params(**case.oracle_split_kw())
    found = 0
    for f, r in enumerate(det):
        k0 = int(r.info["blob_begin"])
        for j, b in enumerate(r.blobs):
            found += assert_blob_equals_oracle(case, sp, r, b, specs[k0 + j], int(presumed[k0 + j]), info[k0 + j], thr[k0 + j])
        assert_per_blob_equal(r, sub[f], case.bg, thr[k0:k0 + len(r.blobs)], case.method, list(case.ranges), case.cm, case.connectivity)
    assert found >= case.min_found
    if case.blobs is not None:
        assert found == sum(b.threshold >= 0 for b in case.blobs)


def test_prefix_call_leaves_the_rest_alone():
    """n_blobs = half of the batch's blobs: the searched prefix equals the oracle like a full call's, the entries past it keep what they held.  Every
    frame of the batch has at most three blobs and one that is searched, so the prefix holds a searched blob whichever frame is pooled first"""
    case = sc.table()["a_mixed_batch"]
    (det, presumed, thr, info, _), specs = search(case, n_search=len(case.blobs) // 2)
    nb, half = len(thr), len(case.blobs) // 2
    assert nb == len(case.blobs) >= 6
    sp = oracle.split_params(**case.oracle_split_kw())
    for r in det:
        k0 = int(r.info["blob_begin"])
        for j, b in enumerate(r.blobs):
            if k0 + j < half:
                assert_blob_equals_oracle(case, sp, r, b, specs[k0 + j], int(presumed[k0 + j]), info[k0 + j], thr[k0 + j])
    assert (thr[half:] == SENTINEL).all() and not np.frombuffer(info[half:].tobytes(), np.uint8).any()
    assert (info[:half]["status"] == 0).any()
