"""trexhip_visual_field_device through the ABI against tests/visual_field_ref.py, byte for byte: depth, ids, points, fov, head distance, all
four layers, all bins, and status.  The scenes (tests/visual_field_scenes.py) are refused when they are built if the restatement calls ONE
of their records fragile, so nothing is masked out of a comparison."""
import ctypes as C
import numpy as np
import pytest
import visual_field_ref as R
import visual_field_scenes as S
from trex_amd import capi

pytestmark = pytest.mark.gpu
FIELDS = ("depth", "ids", "points", "fov", "head_distance", "status")


@pytest.fixture(scope="module")
def seg():
    s = capi.Segmenter(capi.default_params(640, 480, max_batch=1))
    yield s
    s.close()


def run(seg, a, outputs=capi.VF_OUTPUTS, max_tess=None):
    return seg.visual_field(a["outline"], a["info"], a["frame_entries"], a["entries"], a["observers"], S.MAXP,
                            max_tess_points=a["max_tess"] if max_tess is None else max_tess, max_d=a["max_d"], max_distance=a["max_distance"],
                            outputs=outputs)


def same(got, want):
    for k in FIELDS:
        g, w = getattr(got, k), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError(f"{k}: {len(bad)} cells differ, first at {bad[:4].tolist()}: got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def test_layouts_and_constants_agree():
    assert capi.VF_ENTRY_DTYPE == R.ENTRY_DTYPE and capi.VF_OBSERVER_DTYPE == R.OBSERVER_DTYPE and capi.POSTURE_INFO_DTYPE == S.INFO_DTYPE
    assert (capi.VF_CHUNK_RECORDS, capi.VF_LDS_RECORDS) == (S.CHUNK_RECORDS, S.LDS_RECORDS)
    assert (capi.VF_RESOLUTION, capi.VF_LAYERS) == (R.RESOLUTION, R.LAYERS)


@pytest.mark.parametrize("name", ["self", "occlude3", "two_frames", "lds_exact", "lds_exceed", "spans"])
def test_device_equals_the_restatement(seg, name):
    a, want, _ = S.scene(name)
    got = run(seg, a)
    assert (got.status == 0).all()
    same(got, want)


def test_default_params(seg):
    vp = seg.default_vf_params()
    assert (vp.max_d, vp.max_distance) == (640.0 ** 2 + 480.0 ** 2, 5.0) and vp.max_tess_points >= vp.max_points >= 1


def test_a_second_call_gives_the_same_bytes(seg):
    a, want, _ = S.scene("two_frames")
    first, second = run(seg, a), run(seg, a)
    for k in FIELDS:
        assert getattr(first, k).tobytes() == getattr(second, k).tobytes(), k
    same(second, want)


@pytest.mark.parametrize("only", FIELDS)
def test_every_output_pointer_null_but_one(seg, only):
    a, want, _ = S.scene("occlude3")
    got = run(seg, a, outputs=(only,))
    for k in FIELDS:
        if k == only:
            assert getattr(got, k).tobytes() == want[k].tobytes()
        else:
            assert getattr(got, k) is None


def test_capacity_flags_the_frame_and_leaves_the_other_complete(seg):
    a, want, _ = S.scene("capacity")                               # cast with max_tess_points 255; a ring of frame 0 needs 256
    got = run(seg, a)
    f0 = a["observers"]["frame"] == 0
    assert f0.any() and (~f0).any()
    assert (got.status[f0] == 2).all() and (got.status[~f0] == 0).all()
    assert (got.depth[f0] == R.INVALID).all() and (got.ids[f0] == -1).all() and (got.points[f0] == 0).all() and (got.fov[f0] == 0).all()
    assert (got.head_distance[f0] == -1).all()
    same(got, want)
    # one more point of capacity and the frame is cast (its second observer sits wherever its old outline put it: status only)
    assert (run(seg, a, outputs=("status",), max_tess=256).status == R.cast(
        a["outline"], a["info"]["n_outline"], a["info"]["tail_index"], a["info"]["head_index"], a["frame_entries"], a["entries"], a["observers"],
        a["max_d"], a["max_distance"], 256)["status"]).all()


def test_observer_without_posture_gets_status_1(seg):
    a, _, _ = S.scene("occlude3")
    b = dict(a)
    b["info"] = a["info"].copy()
    b["info"]["tail_index"][a["entries"]["posture_row"][0]] = -1
    want = S.reference(b)
    assert want["status"].tolist() == [1]
    same(run(seg, b), want)


def raw_call(seg, a, n_frames=None, n_entries=None, n_observers=None, max_points=S.MAXP, max_tess=S.MAX_TESS, entries=None, observers=None,
             frame_entries=None):
    """the C entry point itself, with counts and tables of the caller's choosing; returns (return code, depth as it stands afterwards)"""
    fe = a["frame_entries"] if frame_entries is None else frame_entries
    en = a["entries"] if entries is None else entries
    ob = a["observers"] if observers is None else observers
    bufs = [np.ascontiguousarray(x) for x in (a["outline"], a["info"], fe, en, ob)]
    dev = []
    for x in bufs:
        d = seg.device_alloc(max(x.nbytes, 16))
        seg.copy_to_device(d, x)
        dev.append(d)
    cells = max(len(ob), 1) * 2 * 2 * 512
    sentinel = np.full(cells, 123.0)
    d_depth = seg.device_alloc(cells * 8)
    seg.copy_to_device(d_depth, sentinel)
    vp = seg.default_vf_params(max_points=max_points, max_tess_points=max_tess, max_d=a["max_d"])
    rc = capi.lib().trexhip_visual_field_device(seg.handle, C.byref(vp), C.c_void_p(dev[0]), C.c_void_p(dev[1]), C.c_void_p(dev[2]),
                                                len(fe) - 1 if n_frames is None else n_frames, C.c_void_p(dev[3]),
                                                len(en) if n_entries is None else n_entries, C.c_void_p(dev[4]),
                                                len(ob) if n_observers is None else n_observers, C.c_void_p(d_depth), None, None, None, None, None)
    depth = seg.copy_to_host(d_depth, (cells,), np.float64)
    for d in dev + [d_depth]:
        seg.device_free(d)
    return rc, depth


def test_refusals(seg):
    a, _, _ = S.scene("two_frames")
    ok, depth = raw_call(seg, a)
    assert ok == 0 and (depth != 123.0).all()
    for kw in (dict(n_frames=-1), dict(n_entries=-1), dict(n_observers=-1), dict(max_points=64, max_tess=63), dict(max_points=0, max_tess=16)):
        rc, depth = raw_call(seg, a, **kw)
        assert rc == -1 and (depth == 123.0).all(), kw                                   # TREXHIP_E_INVALID, nothing written
    lo, hi = int(a["frame_entries"][1]), int(a["frame_entries"][2])
    for entry in (lo - 1, hi, -1, 10 ** 6):                                               # outside frame 1's range
        ob = a["observers"].copy()
        k = int(np.flatnonzero(ob["frame"] == 1)[0])
        ob["entry"][k] = entry
        rc, depth = raw_call(seg, a, observers=ob)
        assert rc == -1 and (depth == 123.0).all(), entry
        assert b"observer" in capi.lib().trexhip_last_error()
    for frame in (-1, 2):
        ob = a["observers"].copy()
        ob["frame"][0] = frame
        rc, depth = raw_call(seg, a, observers=ob)
        assert rc == -1 and (depth == 123.0).all(), frame
    fe = a["frame_entries"].copy()
    fe[1] = fe[2] + 1                                                                     # offsets that do not ascend
    rc, depth = raw_call(seg, a, frame_entries=fe)
    assert rc == -1 and (depth == 123.0).all()
    # nothing to do is not an error
    assert raw_call(seg, a, n_observers=0)[0] == 0
    with pytest.raises(capi.TrexHipError):
        seg.visual_field(a["outline"], a["info"], a["frame_entries"], a["entries"], a["observers"], S.MAXP, max_tess_points=S.MAXP - 1)
