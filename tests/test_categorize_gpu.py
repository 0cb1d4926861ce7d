"""Categorisation on the GPU (the category network of cnn_arch.hip in the context's second slot, k_cat_label, the tracklet vote of categorize.hip)
against the reference's own vectors (tests/golden/category.npz), the float64 restatement (tests/category_ref.py) and the vote's restatement.
Bars as in test_cnn_arch_gpu.py: 1e-4 on softmax, 2e-3 on logits against the reference; logits within 8 x e32 of float64."""
import numpy as np
import pytest
import torch
from trex_amd import capi, synth, weights
import category_cases as cc
import category_ref as cr

pytestmark = pytest.mark.gpu

EXACT_MODES = [capi.CNN_FP32, capi.CNN_BF16X6, capi.CNN_FP16X3]
CHUNK_MAX = 1 << 16         # ARCH_CHUNK_MAX: crops per chunk of the generic chain at small sizes


def make_ctx():
    return capi.Segmenter(capi.default_params(64, 64, max_batch=1))


def run_device(seg, crops, cats, probs=True, logits=True):
    n = crops.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(crops)).cuda()
    lab = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    p = torch.empty((n, cats), dtype=torch.float32, device="cuda") if probs else None
    lg = torch.empty((n, cats), dtype=torch.float32, device="cuda") if logits else None
    seg.categorize_device(d.data_ptr(), n, lab.data_ptr(), p.data_ptr() if probs else None, lg.data_ptr() if logits else None)
    seg.synchronize()
    return lab.cpu().numpy(), p.cpu().numpy() if probs else None, lg.cpu().numpy() if logits else None


def identity_net(seg, classes=6, size=24):
    st = weights.synthetic_state(classes, 5, 1, size, size, arch="v100")
    seg.load_weights(weights.pack_blob(st, classes, 1, size, size, arch="v100"))
    return weights.synthetic_crops(9, 6, 1, size, size)


# ---- 1. the reference's vectors, 2. float64 ----
@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_reference_vectors_and_float64(case):
    (w, h, ch, cats), _, _ = case
    st, fx, pre = cc.state(case), cc.fixture(), f"case/{cc.case_id(case)}/"
    seg = make_ctx()
    id_crops = identity_net(seg)
    seg.probabilities(id_crops)
    guard0 = seg.guard_stats()
    seg.load_category_weights(cc.blob(case))
    assert seg.category_info() == (cats, ch, w, h)
    for n in cc.BATCHES:
        crops = cc.crops(case, n)
        _, l64, lab64 = cr.forward(st, crops, torch.float64)
        _, l32, _ = cr.forward(st, crops, torch.float32)
        e32 = float(np.abs(l32 - l64).max())
        for mode in EXACT_MODES:
            seg.set_identity_precision(mode)
            lab, p, lg = run_device(seg, crops, cats)
            host = seg.categorize(crops)
            lab_only, _, _ = run_device(seg, crops, cats, probs=False, logits=False)
            dp, dl = float(np.abs(p - fx[pre + f"probs/{n}"]).max()), float(np.abs(lg - fx[pre + f"logits/{n}"]).max())
            ratio = float(np.abs(lg - l64).max()) / e32
            print(cc.case_id(case), "mode", mode, "n", n, "softmax", dp, "logits", dl, f"float64: {ratio:.3g} x e32 (e32 = {e32:.3g})")
            assert np.all(np.isfinite(p)) and np.all(np.isfinite(lg)) and np.allclose(p.sum(1), 1.0, atol=1e-5)
            assert dp <= 1e-4 and dl <= 2e-3, (mode, n, dp, dl)
            assert np.array_equal(lab, fx[pre + f"labels/{n}"]), (mode, n)
            assert np.array_equal(host, lab) and np.array_equal(lab_only, lab), (mode, n)
            assert ratio <= cc.LOGIT_FACTOR, (mode, n, ratio, e32)
            assert np.array_equal(lab, lab64), (mode, n)                       # none undecided: test_category_ref.py
            assert np.array_equal(lab, lg.argmax(1))
    seg.set_identity_precision(capi.CNN_FP16X3)
    assert seg.guard_stats() == guard0                                         # the identity network's counters saw no category call
    seg.close()


# ---- the label is the FIRST maximum ----
def test_label_is_the_first_maximum():
    w = h = 8
    cats = 200
    st = weights.synthetic_category_state(cats, 3, 1, w, h)
    st["fc2.weight"][:] = 0
    b = np.linspace(-1, 0, cats).astype(np.float32)
    b[[3, 70, 199]] = 2.5                                                     # three equal maxima, in two repetitions of the scan and two lanes of one
    st["fc2.bias"] = b
    seg = make_ctx()
    seg.load_category_weights(weights.pack_category_blob(st, cats, 1, w, h))
    lab, p, lg = run_device(seg, weights.synthetic_crops(5, 1, 1, w, h), cats)
    assert np.array_equal(lg, np.tile(b, (5, 1))) and np.array_equal(lab, np.full(5, 3, np.int32))
    st["fc2.bias"] = np.zeros(cats, np.float32)                                # every logit equal: category 0
    seg.load_category_weights(weights.pack_category_blob(st, cats, 1, w, h))
    assert np.array_equal(run_device(seg, weights.synthetic_crops(5, 1, 1, w, h), cats)[0], np.zeros(5, np.int32))
    seg.close()


# ---- 3. chunks and the range guard ----
def _loud_state(w, h, cats):
    """weights whose first block leaves the fp16 range on a white crop and stays far inside it on a mid-grey one: no bias in block 1, so its output is
    proportional to the normalised input, and a BatchNorm2d scale of 3e5"""
    st = weights.synthetic_category_state(cats, 9, 1, w, h)
    st["conv1.bias"][:] = 0
    st["batch_norm1.bias"][:] = 0
    st["batch_norm1.weight"] = (st["batch_norm1.weight"] * 3e5).astype(np.float32)
    return st


def test_chunks_and_loud_crops():
    w = h = 8
    cats = 3
    st = _loud_state(w, h, cats)
    n = CHUNK_MAX + 3
    rng = np.random.default_rng(12)
    crops = rng.integers(124, 132, (n, h, w, 1), dtype=np.uint8)
    loud = [0, CHUNK_MAX - 1, CHUNK_MAX, n - 1]                                # both sides of the chunk boundary
    crops[loud] = 255
    # on the CPU: the guard CAN be reached with normalised inputs -- the weights decide -- and these crops stand on both sides of the fp16 range
    probe = np.concatenate([crops[loud], crops[1:200]])
    a1 = cr.trunk(st, cr.normalise(probe, torch.float64), torch.float64, upto=1).flatten(1).abs().max(1).values.numpy()
    assert a1[:4].min() > 1.1 * 65504 and a1[4:].max() < 0.5 * 65504, (a1[:4], a1[4:].max())
    seg = make_ctx()
    seg.load_category_weights(weights.pack_category_blob(st, cats, 1, w, h))
    lab, p, lg = run_device(seg, crops, cats)                                  # FP16X3, the default
    la, pa, lga = run_device(seg, crops[:CHUNK_MAX], cats)
    lb, pb, lgb = run_device(seg, crops[CHUNK_MAX:], cats)
    assert lab.tobytes() == la.tobytes() + lb.tobytes() and p.tobytes() == pa.tobytes() + pb.tobytes() and lg.tobytes() == lga.tobytes() + lgb.tobytes()
    for r in loud + [1, CHUNK_MAX - 2, CHUNK_MAX + 1]:                         # one crop's row does not depend on n
        l1, p1, lg1 = run_device(seg, crops[r:r + 1], cats)
        assert l1[0] == lab[r] and p1.tobytes() == p[r:r + 1].tobytes() and lg1.tobytes() == lg[r:r + 1].tobytes(), r
    assert np.all(np.isfinite(lg)) and np.all(np.isfinite(p))
    seg.set_identity_precision(capi.CNN_BF16X6)                                # a crop outside the fp16 range is re-run by the BF16X6 kernels
    _, p6, lg6 = run_device(seg, crops[loud], cats)
    assert lg6.tobytes() == lg[loud].tobytes() and p6.tobytes() == p[loud].tobytes()
    some = loud + [1, 2, 3]
    _, l64, _ = cr.forward(st, crops[some], torch.float64)
    _, l32, _ = cr.forward(st, crops[some], torch.float32)
    e32 = float(np.abs(l32 - l64).max())
    ratio = float(np.abs(lg[some] - l64).max()) / e32
    print(f"loud crops: {ratio:.3g} x e32 (e32 = {e32:.3g}, max |logit| = {np.abs(l64).max():.3g})")
    assert ratio <= cc.LOGIT_FACTOR, (ratio, e32)
    seg.close()


# ---- 4. two networks in one context ----
def test_two_networks_in_one_context():
    seg = make_ctx()
    id_crops = identity_net(seg)
    p0 = seg.probabilities(id_crops)
    small, large = cc.CASES[1], cc.CASES[4]
    crops_s, crops_l = cc.crops(small, 37), cc.crops(large, 37)
    seg.load_category_weights(cc.blob(small))
    assert seg.probabilities(id_crops).tobytes() == p0.tobytes()               # loading the category network
    ls = seg.categorize(crops_s)
    assert seg.probabilities(id_crops).tobytes() == p0.tobytes()               # ... and calling it
    id_crops = identity_net(seg)                                               # reloading the identity network keeps the category network
    assert seg.category_info() == small[0][3:] + small[0][2:3] + small[0][:2]
    assert np.array_equal(seg.categorize(crops_s), ls)
    assert seg.probabilities(id_crops).tobytes() == p0.tobytes()
    seg.load_category_weights(cc.blob(large))                                  # small -> large -> small
    ll = seg.categorize(crops_l)
    assert np.array_equal(ll, cc.fixture()[f"case/{cc.case_id(large)}/labels/37"])
    assert seg.probabilities(id_crops).tobytes() == p0.tobytes()
    seg.load_category_weights(cc.blob(small))
    assert np.array_equal(seg.categorize(crops_s), ls) and np.array_equal(ls, cc.fixture()[f"case/{cc.case_id(small)}/labels/37"])
    assert np.array_equal(seg.categorize(crops_s[:3]), ls[:3])
    assert seg.probabilities(id_crops).tobytes() == p0.tobytes()
    seg.close()
    seg = make_ctx()                                                           # the reverse: the category network first
    seg.load_category_weights(cc.blob(small))
    assert np.array_equal(seg.categorize(crops_s), ls)
    id_crops = identity_net(seg)
    assert seg.probabilities(id_crops).tobytes() == p0.tobytes() and np.array_equal(seg.categorize(crops_s), ls)
    seg.close()


# ---- 5. the vote ----
def _vote_rows(n, T, C, seed, one_tracklet=False):
    rng = np.random.default_rng(seed)
    labels = rng.integers(-1, C + 2, n).astype(np.int32)                       # -1: none; C, C + 1: skipped and counted
    labels[rng.random(n) < 0.05] = -3
    tracklet = np.zeros(n, np.int32) if one_tracklet else rng.integers(0, T, n).astype(np.int32)
    return labels, tracklet


VOTES = [(1, 1, 1, False), (1, 7, 3, False), (100003, 1, 4, False), (100003, 7, 4, False), (100003, 65536, 2, False), (100003, 7, 1, False),
         (100003, 7, 70, False), (100003, 7, 1024, False), (100003, 3, 1024, False), (100003, 58, 70, False), (100003, 57, 70, False), (100003, 5, 4, True),
         (100003, 9, 1024, True)]


@pytest.mark.parametrize("n,T,C,one", VOTES, ids=[f"n{n}-T{T}-C{C}{'-one' if o else ''}" for n, T, C, o in VOTES])
def test_vote_equals_the_restatement(n, T, C, one):
    labels, tracklet = _vote_rows(n, T, C, n + 31 * T + C, one)
    counts, rows, label, share, skipped = cr.vote(labels, tracklet, T, C)
    seg = make_ctx()
    got = seg.tracklet_labels(labels, tracklet, T, C)
    assert got.counts.tobytes() == counts.tobytes() and got.rows.tobytes() == rows.tobytes() and got.label.tobytes() == label.tobytes()
    assert got.share.tobytes() == share.tobytes() and got.skipped == skipped
    assert int(rows.sum()) == n
    no_share = seg.tracklet_labels(labels, tracklet, T, C, share=False)
    assert no_share.share is None and no_share.label.tobytes() == label.tobytes() and no_share.skipped == skipped
    seg.close()


def test_vote_hand_cases_and_refusals():
    seg = make_ctx()
    got = seg.tracklet_labels([2, 0, 2, 0, -1, 5, 1], [1, 1, 1, 1, 1, 1, 3], 4, 3)      # a tie: the lowest index; tracklets 0 and 2 are empty
    assert got.label.tolist() == [-1, 0, -1, 1] and got.rows.tolist() == [0, 6, 0, 1] and got.skipped == 1
    assert got.counts.tolist() == [[0, 0, 0], [2, 0, 2], [0, 0, 0], [0, 1, 0]]
    assert got.share[1].tobytes() == (np.array([2, 0, 2], np.float32) / np.float32(6)).tobytes() and not got.share[[0, 2]].any()
    got = seg.tracklet_labels([-1, -1, 9], [0, 0, 0], 1, 3)                             # all rows unlabelled or out of range
    assert got.label.tolist() == [-1] and got.rows.tolist() == [3] and got.skipped == 1 and not got.share.any()
    assert seg.tracklet_labels([], [], 3, 2).label.tolist() == [-1, -1, -1]            # n = 0: a no-op
    # an out-of-range tracklet id: refused, the outputs untouched
    n, T, C = 5000, 6, 4
    labels, tracklet = _vote_rows(n, T, C, 3)
    for bad in (T, -1, 1 << 30):
        tr = tracklet.copy()
        tr[n - 7] = bad
        d = [torch.from_numpy(labels).cuda(), torch.from_numpy(tr).cuda()]
        outs = [torch.full((T, C), 77, dtype=torch.int32, device="cuda"), torch.full((T,), 77, dtype=torch.int32, device="cuda"),
                torch.full((T,), 77, dtype=torch.int32, device="cuda"), torch.full((T, C), 77.0, dtype=torch.float32, device="cuda")]
        with pytest.raises(capi.TrexHipError, match="tracklet id") as e:
            seg.tracklet_labels_device(d[0].data_ptr(), d[1].data_ptr(), n, T, C, *[o.data_ptr() for o in outs])
        assert e.value.code == -1
        assert all(bool((o == 77).all()) for o in outs)
    for T_, C_ in ((0, 3), (3, 0), (3, 1025)):
        with pytest.raises(capi.TrexHipError) as e:
            seg.tracklet_labels(labels, tracklet % 3, T_, C_)
        assert e.value.code == -1
    seg.close()


# ---- 6. end to end: frames -> blobs -> crops -> categories -> one label per blob index ----
def test_end_to_end_from_frames():
    fr, bg = synth.batch("C2", 16)
    n, H, W = fr.shape
    case = cc.CASES[4]                                                         # 80 x 80 x 1, the crops trexhip_crops_device makes by default
    (w, h, ch, cats), _, _ = case
    seg = capi.Segmenter(capi.default_params(W, H, max_batch=n))
    seg.set_background(bg)
    seg.load_category_weights(cc.blob(case))
    seg.segment_device(torch.from_numpy(fr).cuda().data_ptr(), n)
    res = seg.fetch()
    per_frame = [len(r.blobs) for r in res]
    nb = sum(per_frame)
    assert nb >= n
    crops = torch.zeros((nb, h, w), dtype=torch.uint8, device="cuda")
    seg.crops_device(crops.data_ptr(), nb)
    lab = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
    seg.categorize_device(crops.data_ptr(), nb, lab.data_ptr())
    tracklet = np.concatenate([np.arange(k, dtype=np.int32) for k in per_frame])      # the blob's frame-local index
    T = max(per_frame)
    d_tr = torch.from_numpy(tracklet).cuda()
    counts = torch.zeros((T, cats), dtype=torch.int32, device="cuda")
    rows, label = torch.zeros(T, dtype=torch.int32, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda")
    share = torch.zeros((T, cats), dtype=torch.float32, device="cuda")
    skipped = seg.tracklet_labels_device(lab.data_ptr(), d_tr.data_ptr(), nb, T, cats, counts.data_ptr(), rows.data_ptr(), label.data_ptr(), share.data_ptr())
    host_crops = crops.cpu().numpy()[..., None]
    assert host_crops.any()
    _, _, want_lab = cr.forward(cc.state(case), host_crops, torch.float32)
    _, l64, lab64 = cr.forward(cc.state(case), host_crops, torch.float64)
    top = np.sort(l64, 1)
    decided = (top[:, -1] - top[:, -2]) > 1e-3                                 # (blob crops are not the seeded cases: a near-tie may go either way)
    got_lab = lab.cpu().numpy()
    assert np.array_equal(got_lab[decided], lab64[decided]) and decided.mean() >= 0.99
    wc, wr, wl, ws, wsk = cr.vote(got_lab, tracklet, T, cats)
    assert counts.cpu().numpy().astype(np.uint32).tobytes() == wc.tobytes() and rows.cpu().numpy().astype(np.uint32).tobytes() == wr.tobytes()
    assert label.cpu().numpy().tobytes() == wl.tobytes() and share.cpu().numpy().tobytes() == ws.tobytes() and skipped == wsk == 0
    if decided.all():
        assert np.array_equal(wl, cr.vote(want_lab, tracklet, T, cats)[2])
    seg.close()


# ---- 7. refusals ----
def test_refusals():
    seg = make_ctx()
    assert seg.category_info() == (0, 0, 0, 0)
    crops = np.zeros((2, 8, 8, 1), np.uint8)
    with pytest.raises(capi.TrexHipError, match="no category weights") as e:
        seg.categorize(crops)
    assert e.value.code == -1
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.TrexHipError, match="no category weights"):
        seg.categorize_device(d.data_ptr(), 2, d.data_ptr())
    good = weights.pack_category_blob(weights.synthetic_category_state(3, 1, 1, 8, 8), 3, 1, 8, 8)
    assert capi.lib().trexhip_categorize_blob_bytes(3, 1, 8, 8) == len(good)
    seg.load_category_weights(good)
    seg.categorize_device(d.data_ptr(), 0, d.data_ptr())                       # n = 0: a no-op
    assert len(seg.categorize(np.zeros((0, 8, 8, 1), np.uint8))) == 0
    want = seg.categorize(crops)
    ident = weights.pack_blob(weights.synthetic_state(3, 1, 1, 8, 8, arch="v100"), 3, 1, 8, 8, arch="v100")
    with pytest.raises(capi.TrexHipError, match="magic"):
        seg.load_category_weights(ident)                                       # an identity blob into the category loader
    with pytest.raises(capi.TrexHipError, match="magic"):
        seg.load_weights(good)                                                 # ... and the reverse
    assert seg.num_classes() == 0

    def hdr(blob, **kw):
        h = np.frombuffer(blob[:32], np.int32).copy()
        for k, v in kw.items():
            h[dict(magic=0, version=1, categories=2, width=3, height=4, channels=5)[k]] = v
        return h.tobytes() + blob[32:]
    for field, bad, code in (("size", good + b"\0\0\0\0", -1), ("size", good[:-4], -1), ("size", good[:16], -1), ("version", hdr(good, version=2), -1),
                             ("width", hdr(good, width=7), -4), ("height", hdr(good, height=7), -4), ("width", hdr(good, width=257), -4),
                             ("channels", hdr(good, channels=2), -4), ("categories", hdr(good, categories=0), -1),
                             ("categories", hdr(good, categories=1025), -1)):
        with pytest.raises(capi.TrexHipError, match=field) as e:
            seg.load_category_weights(bad)
        assert e.value.code == code, (field, e.value.code)
        assert seg.category_info() == (3, 1, 8, 8) and np.array_equal(seg.categorize(crops), want)      # the loaded network stays
    for args in ((3, 1, 7, 8), (3, 1, 8, 257), (3, 2, 8, 8), (0, 1, 8, 8), (1025, 1, 8, 8)):
        assert capi.lib().trexhip_categorize_blob_bytes(*args) == 0
    with pytest.raises(ValueError):
        seg.categorize(np.zeros((2, 8, 8, 3), np.uint8))                       # crops of another channel count than the network's
    seg.close()
