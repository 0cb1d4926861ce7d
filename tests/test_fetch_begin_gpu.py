"""trexhip_fetch_begin / trexhip_fetch_wait: trexhip_fetch in two halves.  fetch_begin returns once the counts and the frame table are on the
host, with the copies of the blob / run / pixel tables queued behind an event; fetch_wait blocks until they have arrived.  Whatever a caller
does in between, the tables must be the bytes of trexhip_fetch on the same batch, and every library call that overwrites the device tables or
the pinned mirrors must wait for the copies itself.

17 frames of a small synthetic scene (320 x 240, 12 ellipses): above the 16 frames up to which one export kernel serves a fetch.

What "the same batch" means: a frame reserves its share of the pooled tables with an atomic add when its labelling ends (k_blobs,
trex_amd/csrc/segment.hip), so two segment calls on the same frames give the same blobs per frame in a pooled ORDER that may differ, and with it
the frame table's *_begin words.  Byte equality is therefore asked of two fetches of ONE segment call; across segment calls the tables are
compared frame by frame (`by_frame`), which is every byte but the pooled order."""
import numpy as np
import pytest
import torch
from trex_amd import capi, synth

pytestmark = pytest.mark.gpu

W, H, NB = 320, 240, 12
N = 17


def scene(n, t0=0):
    bg = synth.background(W, H)
    return np.stack([synth.frame(W, H, NB, 3, t0 + t, bg) for t in range(n)]), bg


def tables(r):
    """the four tables behind a BatchResult, as bytes (copied out of the pinned mirrors now)"""
    pc = int(r.pixel_channels) or 1
    return (capi._from_addr(r.frames, r.n_frames, capi.INFO_DTYPE).tobytes(), capi._from_addr(r.blobs, r.total_blobs, capi.BLOB_DTYPE).tobytes(),
            capi._from_addr(r.runs, r.total_runs, capi.RUN_DTYPE).tobytes(), capi._from_addr(r.pixels, r.total_pixels * pc, np.dtype(np.uint8)).tobytes(),
            (int(r.n_frames), int(r.total_blobs), int(r.total_runs), int(r.total_pixels)))


def by_frame(t):
    """the tables of `tables()` frame by frame, without the pooled order: per frame its counts and flags and its own slices of the three tables
    (a blob's run_begin / pix_begin are frame-relative)"""
    info = np.frombuffer(t[0], capi.INFO_DTYPE)
    blobs, runs, px = np.frombuffer(t[1], capi.BLOB_DTYPE), np.frombuffer(t[2], capi.RUN_DTYPE), np.frombuffer(t[3], np.uint8)
    out = []
    for f in info:
        b0, r0, p0 = int(f["blob_begin"]), int(f["run_begin"]), int(f["pix_begin"])
        nb, nr, npx = int(f["n_blobs"]), int(f["n_runs"]), int(f["n_pixels"])
        if f["flags"]:
            out.append((int(f["flags"]),))
            continue
        out.append((nb, nr, npx, int(f["n_raw_runs"]), int(f["n_raw_blobs"]), blobs[b0:b0 + nb].tobytes(), runs[r0:r0 + nr].tobytes(), px[p0:p0 + npx].tobytes()))
    return out


@pytest.fixture(scope="module")
def batches():
    """two batches of 17 frames on the device, the background, and each batch's tables frame by frame from a plain fetch"""
    fa, bg = scene(N)
    fb, _ = scene(N, t0=100)
    da, db = torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda()
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=N))
    seg.set_background(bg)
    want = []
    for d in (da, db):
        seg.segment_device(d.data_ptr(), N)
        want.append(by_frame(tables(seg.fetch_raw())))
    seg.close()
    assert sum(f[0] for f in want[0]) >= N * NB // 2 and want[0] != want[1]
    return da, db, bg, want


def context(bg, **kw):
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=N, **kw))
    seg.set_background(bg)
    return seg


def crops_of(seg, n):
    crops = torch.zeros((n, 80, 80), dtype=torch.uint8, device="cuda")
    seg.crops_device(crops.data_ptr(), n)
    seg.synchronize()
    return crops.cpu().numpy().tobytes()


def test_begin_and_wait_give_the_tables_of_fetch(batches):
    da, db, bg, want = batches
    seg = context(bg)
    seg.fetch_wait()                                          # nothing pending, no batch yet
    seg.segment_device(da.data_ptr(), N)
    r = seg.fetch_begin_raw()
    assert seg.last_fetch_rc == 0
    early = tables(r)                                         # counts and frame table: there at once
    seg.fetch_wait()
    got = tables(r)
    assert got[0] == early[0] and got[4] == early[4]
    seg.fetch_wait()                                          # twice
    assert tables(r) == got
    assert tables(seg.fetch_raw()) == got                     # trexhip_fetch on the same batch: byte for byte
    assert by_frame(got) == want[0]                           # ... and, frame by frame, another segment call's
    seg.close()


def test_crops_between_begin_and_wait(batches):
    da, db, bg, want = batches
    seg = context(bg)
    own = torch.cuda.Stream()
    seg.segment_device(da.data_ptr(), N)
    r = seg.fetch_begin_raw()
    seg.set_stream(own.cuda_stream)                           # as the pipelined lanes do: the copies stay on the stream they were queued on
    n = int(r.total_blobs)
    crops = torch.zeros((n, 80, 80), dtype=torch.uint8, device="cuda")
    seg.crops_device(crops.data_ptr(), n)                     # queued with the copies pending
    seg.fetch_wait()
    seg.synchronize()
    got = tables(r)
    assert tables(seg.fetch_raw()) == got
    assert crops.cpu().numpy().tobytes() == crops_of(seg, n)  # the same batch's crops behind a plain fetch
    seg.close()


def test_a_segment_call_with_a_fetch_pending(batches):
    """the caller forgets fetch_wait: the next detect pass waits itself before it overwrites the tables, so the mirrors hold batch A whole"""
    da, db, bg, want = batches
    seg = context(bg)
    seg.segment_device(da.data_ptr(), N)
    ra = seg.fetch_begin_raw()
    seg.segment_device(db.data_ptr(), N)
    assert by_frame(tables(ra)) == want[0]
    rb = seg.fetch_begin_raw()
    got = tables(seg.fetch_raw())                             # a plain fetch with a fetch pending: the same batch, complete
    assert by_frame(got) == want[1]
    seg.fetch_wait()
    assert tables(rb) == got
    seg.close()


def test_over_capacity_returns_the_same_code_and_message(batches):
    da, db, bg, want = batches
    seg = context(bg, max_blobs=NB // 2)
    seg.segment_device(da.data_ptr(), N)
    r1 = seg.fetch_begin_raw()
    rc1, msg1 = seg.last_fetch_rc, seg.last_capacity_error
    seg.fetch_wait()
    t1 = tables(r1)
    r0 = capi.BatchResult()
    rc0, msg0 = capi.lib().trexhip_fetch(seg._h, capi.C.byref(r0)), capi.lib().trexhip_last_error().decode()
    assert rc0 == rc1 == -3 and msg0 == msg1 and "exceeded capacity" in msg0
    assert tables(r0) == t1
    seg.close()


@pytest.mark.parametrize("n", [16, 0])
def test_small_and_empty_batches_are_a_plain_fetch(batches, n):
    da, db, bg, want = batches
    seg = context(bg)
    seg.segment_device(da.data_ptr(), n)
    r = seg.fetch_begin_raw()
    got = tables(r)                                           # complete without a wait: nothing is pending
    assert got[4][0] == n
    assert tables(seg.fetch_raw()) == got
    seg.fetch_wait()
    assert tables(r) == got
    if n:
        assert by_frame(got) == want[0][:n]
    seg.close()
