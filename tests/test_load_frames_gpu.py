"""trexhip_load_frames_v6_device (trex_amd/csrc/unpack.hip): stored V_6 frame bodies become the context's last batch, and the track stage
runs on them unchanged.  Everything is compared byte for byte: (1) the loaded tables against the oracle, no device segmentation involved;
(2) a round trip through the library -- segment + pack on one context, load on another whose frame image holds stale pixels -- with
re-threshold, crops, transformed crops, posture and the split search on both; (3) a frame beyond capacity and a malformed frame fail
alone; (4) the refusals.  The bounds rules the device applies are those of trex_amd/csrc/pv_read.h, which tests/test_pv_read.py runs on
the same malformed bodies under the host sanitizers."""
import numpy as np
import pytest
from oracle import oracle
from trex_amd import capi, synth
import pv_cases
from pv_cases import W, H

pytestmark = pytest.mark.gpu


def _upload(bodies):
    """bodies back to back (the 11-byte frame heads put them at odd offsets) -> (device bytes, device offsets, host offsets)"""
    import torch
    off = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int64)
    cat = np.concatenate([np.asarray(b, np.uint8) for b in bodies] + [np.zeros(1, np.uint8)])
    return torch.from_numpy(cat).cuda(), torch.from_numpy(off).cuda(), off


def _load(seg, bodies, want_ts=False):
    import torch
    d, o, _ = _upload(bodies)
    ts = torch.full((len(bodies),), -1, dtype=torch.int64, device="cuda") if want_ts else None
    seg.load_frames_v6_device(d.data_ptr(), o.data_ptr(), len(bodies), ts.data_ptr() if want_ts else 0)
    return ts


def _assert_tables(r, ob, orr, opx, what):
    assert r.runs.tobytes() == orr.tobytes(), what
    assert r.pixels.tobytes() == opx.tobytes(), what
    assert len(r.blobs) == len(ob), what
    for name in ob.dtype.names:
        assert np.array_equal(r.blobs[name], ob[name]), (what, name)
    assert r.blobs.tobytes() == ob.tobytes(), what


def _painted(blob_lines, seed):
    """frame and background in which oracle.segment finds exactly these blobs"""
    rng = np.random.default_rng(seed)
    bg = np.full((H, W), 200, np.uint8)
    fr = bg.copy()
    for lines in blob_lines:
        for x0, x1, y in lines:
            fr[y, x0:x1 + 1] = rng.integers(10, 150, x1 - x0 + 1)
    return fr, bg


def _oracle_frames():
    out = [pv_cases.scene(s) for s in (0, 1)]
    e = pv_cases.scene(0)
    out.append((e[0][:0], e[1][:0], e[2][:0]))                                              # an empty frame in the middle
    out.append(pv_cases.scene(2))
    singles = [[(2 * (i % 150), 2 * (i % 150), 2 * (i // 150))] for i in range(300)]     # 300 isolated pixels: more blobs than any per-workgroup chunk
    comb = [(0, 298, 10)] + [(2 * i, 2 * i, 11) for i in range(150)] + [(2 * i, 2 * i, 12) for i in range(149)]   # one blob of 300 lines, 150 on one row
    corner = [(315, 319, 94), (310, 319, 95)]                                               # touches x = W - 1, y = H - 1
    for k, blob_lines in enumerate((singles, [comb, corner])):
        fr, bg = _painted(blob_lines, 40 + k)
        b, r, px = oracle.segment(fr, bg, oracle.make_params(W, H))
        assert list(b["n_runs"]) == [len(l) for l in blob_lines]
        out.append((b, r, px))
    return out


def test_tables_equal_the_oracle():
    frames = _oracle_frames()
    n = len(frames)
    ts = np.arange(n, dtype=np.uint64) * 33333 + 0x0102030405060708
    bodies = [oracle.pv_serialize_v6(b, r, px, int(t)) for (b, r, px), t in zip(frames, ts)]
    assert any(int(o) % 2 for o in np.cumsum([len(b) for b in bodies]))                     # bodies at odd offsets
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=n, max_blobs=512))
    got_ts = _load(seg, bodies, want_ts=True)
    res = seg.fetch()
    assert np.array_equal(got_ts.cpu().numpy().astype(np.uint64), ts)
    bb = rb = pb = 0
    for f, (r, (b, rr, px)) in enumerate(zip(res, frames)):
        _assert_tables(r, b, rr, px, f)
        i = r.info
        assert i["flags"] == 0 and i["reserved"][0] == 0 and i["n_raw_runs"] == len(rr) and i["n_raw_blobs"] == len(b)
        assert (i["n_blobs"], i["n_runs"], i["n_pixels"]) == (len(b), len(rr), len(px))
        assert (i["blob_begin"], i["run_begin"], i["pix_begin"]) == (bb, rb, pb)             # pooled in frame order
        bb += len(b); rb += len(rr); pb += len(px)
    raw = seg.fetch_raw()
    assert (raw.total_blobs, raw.total_runs, raw.total_pixels) == (bb, rb, pb)
    seg.close()


# ---- round trip through the library, track stage included -----------------------------------------------------------------------------
def _track_stage(seg, res):
    """every track-stage output of the context's batch, keyed by (frame, index in frame): the two contexts pool frames differently"""
    import torch
    total = sum(len(r.blobs) for r in res)
    begin = [int(r.info["blob_begin"]) for r in res]
    keys = {begin[f] + k: (f, k) for f, r in enumerate(res) for k in range(len(r.blobs))}
    out = {}
    seg.rethreshold(25, method=0)
    for f, s in enumerate(seg.fetch(rethreshold=True)):
        b = s.blobs.copy()
        b["parent"] -= begin[f]                                                            # pooled index of the detect blob -> its index in the frame
        out["rethreshold", f] = (b.tobytes(), s.runs.tobytes(), s.pixels.tobytes())

    assert sum(len(v[0]) for key, v in out.items()) > 0

    def per_blob(name, a):
        a = a.cpu().numpy()
        for i, key in keys.items():
            out[(name,) + key] = a[i].tobytes()

    for difference in (0, 1):
        crops = torch.full((total, 80, 80), 77, dtype=torch.uint8, device="cuda")
        seg.crops_device(crops.data_ptr(), total, 80, 80, difference=difference)
        per_blob("crops%d" % difference, crops)
    tr = np.zeros((total, 6), np.float32); ln = np.zeros(total, np.float32)
    for i, (f, k) in keys.items():                                                         # moments transforms taken from the blob sums
        B = res[f].blobs[k]
        npx = float(B["n_pixels"]); cx, cy = float(B["m10"]) / npx, float(B["m01"]) / npx
        mu20, mu02, mu11 = float(B["m20"]) / npx - cx * cx, float(B["m02"]) / npx - cy * cy, float(B["m11"]) / npx - cx * cy
        a = 0.5 * np.arctan2(2 * mu11, mu20 - mu02); cs, sn = np.cos(a), np.sin(a)
        ox, oy = cx - float(B["x0"]), cy - float(B["y0"])
        tr[i] = [cs, sn, -(cs * ox + sn * oy), -sn, cs, -(-sn * ox + cs * oy)]
        ln[i] = 10.0 + float(B["x1"]) - float(B["x0"])
    crops = torch.full((total, 80, 80), 77, dtype=torch.uint8, device="cuda")
    seg.crops_transformed_device(crops.data_ptr(), tr, ln)
    per_blob("transformed", crops)
    MP = 512
    outline = torch.zeros((total, MP, 2), dtype=torch.float32, device="cuda")
    segs = torch.zeros((total, MP // 2 + 1, 4), dtype=torch.float32, device="cuda")
    info = torch.zeros((total, 8), dtype=torch.int32, device="cuda")
    seg.posture_device(total, outline.data_ptr(), segs.data_ptr(), info.data_ptr(), max_points=MP)
    per_blob("outline", outline); per_blob("segments", segs); per_blob("posture_info", info)
    d_pres = torch.full((total,), 2, dtype=torch.int32, device="cuda")
    d_thr = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    d_info = torch.zeros((total, capi.SPLIT_INFO_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    seg.split_search_device(d_pres.data_ptr(), total, d_thr.data_ptr(), d_info.data_ptr(), method=0)
    per_blob("split_threshold", d_thr); per_blob("split_info", d_info)
    seg.synchronize()
    return out


@pytest.mark.parametrize("invert", [0, 1])
def test_round_trip_through_the_library(invert):
    import torch
    fr, bg = synth.batch("C2", 5)
    fr = fr.copy()
    n, FH, FW = fr.shape
    fr[3] = bg                                                                             # one frame set to the background
    a = capi.Segmenter(capi.default_params(FW, FH, max_batch=n, image_invert=invert))     # under image_invert the inverted frames: the same blobs
    a.set_background(bg)
    d = torch.from_numpy(255 - fr if invert else fr).cuda()
    a.segment_device(d.data_ptr(), n)
    res_a = a.fetch()
    assert sum(len(r.blobs) for r in res_a) > 0 and len(res_a[3].blobs) == 0
    ts = np.arange(n, dtype=np.uint64) * 40000 + 9
    cap = sum(11 + 4 * len(r.blobs) + 4 * len(r.runs) + len(r.pixels) for r in res_a) + 64
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda"); off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    a.pack_frames_v6_device(out.data_ptr(), out.numel(), off.data_ptr(), ts)
    a.synchronize()

    b = capi.Segmenter(capi.default_params(FW, FH, max_batch=n))                           # image_invert stays 0 here: stored pixels are final
    b.set_background(bg)
    other, _ = synth.batch("C2", n, t0=7)
    b.segment_host(list(other))                                                            # leaves stale pixels in the context's frame image
    b.fetch()
    got_ts = torch.zeros(n, dtype=torch.int64, device="cuda")
    b.load_frames_v6_device(out.data_ptr(), off.data_ptr(), n, got_ts.data_ptr())
    res_b = b.fetch()
    assert np.array_equal(got_ts.cpu().numpy().astype(np.uint64), ts)
    for f in range(n):
        _assert_tables(res_b[f], res_a[f].blobs, res_a[f].runs, res_a[f].pixels, f)
    ta, tb = _track_stage(a, res_a), _track_stage(b, res_b)
    assert ta.keys() == tb.keys()
    for key in ta:
        assert ta[key] == tb[key], key
    a.close(); b.close()


# ---- capacity and malformed frames fail alone -------------------------------------------------------------------------------------------
def _crops_of(seg, res, f):
    import torch
    total = sum(len(r.blobs) for r in res)
    crops = torch.full((total, 80, 80), 77, dtype=torch.uint8, device="cuda")
    seg.crops_device(crops.data_ptr(), total, 80, 80)
    seg.synchronize()
    b0 = int(res[f].info["blob_begin"])
    return crops.cpu().numpy()[b0:b0 + len(res[f].blobs)].tobytes()


@pytest.mark.parametrize("case", ["x1_is_width", pv_cases.CUT_INSIDE_PIXELS])
def test_capacity_and_malformed_frames_fail_alone(case):
    frames = _oracle_frames()
    many, good = frames[4], frames[5]                                                      # 300 blobs: over max_blobs below; the comb and the corner blob
    assert len(many[0]) == 300 and len(good[0]) == 2
    bodies = [oracle.pv_serialize_v6(*many, 1), pv_cases.malformed_cases()[case], oracle.pv_serialize_v6(*good, 3)]
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=3, max_blobs=256))
    seg.set_background(np.full((H, W), 200, np.uint8))
    _load(seg, bodies)
    with pytest.raises(capi.TrexHipError) as e:
        seg.fetch()
    assert e.value.code == -1 and "malformed" in str(e.value) and "frame 1 " in str(e.value)
    res = e.value.frames
    assert res[0].info["flags"] == capi.FRAME_OVERFLOW_OUTPUT and res[1].info["flags"] == capi.FRAME_MALFORMED and res[2].info["flags"] == 0
    assert len(res[0].blobs) == len(res[1].blobs) == 0 and res[0].info["n_blobs"] == res[1].info["n_blobs"] == 0
    _assert_tables(res[2], *good, "the good frame")
    crops = _crops_of(seg, res, 2)
    # without the malformed frame the capacity error is reported as it always was
    _load(seg, [bodies[0], bodies[2]])
    res2 = seg.fetch()
    assert "exceeded capacity" in seg.last_capacity_error and res2[0].info["flags"] == capi.FRAME_OVERFLOW_OUTPUT
    _assert_tables(res2[1], *good, "beside the overflow")
    # the good frame loaded alone: the same crops
    _load(seg, [bodies[2]])
    alone = seg.fetch()
    _assert_tables(alone[0], *good, "alone")
    assert _crops_of(seg, alone, 0) == crops
    seg.close()


def test_refusals_without_a_launch():
    import torch
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=2))
    d, o, _ = _upload([pv_cases.two_blob_body()])
    for args in ((d.data_ptr(), o.data_ptr(), 0), (d.data_ptr(), o.data_ptr(), 3), (0, o.data_ptr(), 1), (d.data_ptr(), 0, 1)):
        with pytest.raises(capi.TrexHipError) as e:
            seg.load_frames_v6_device(*args)
        assert e.value.code == -1, args
    seg.close()
    col = capi.Segmenter(capi.default_params(W, H, max_batch=2, pixel_encoding=capi.ENC_RGB8))
    with pytest.raises(capi.TrexHipError) as e:
        col.load_frames_v6_device(d.data_ptr(), o.data_ptr(), 1)
    assert e.value.code == -4
    col.close()
