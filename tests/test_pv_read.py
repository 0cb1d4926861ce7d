"""Reading stored .pv frames back, host side (no GPU): the layout and bounds rules of trex_amd/csrc/pv_read.h -- the ones the device loader
(trex_amd/csrc/unpack.hip) applies --, the data-section reader and LZO1X decoder of trex_amd/csrc/pvfile.cpp, and the body writer of
trex_amd/host/HipTrackFrames.h.  tests/cpp/test_pv_read.cpp drives them as a stand-alone program, built plainly and a second time with
-fsanitize=address,undefined (host code only, never loaded into Python); everything is compared byte for byte with the oracle's
restatement of pv::Frame::serialize / read_from (oracle/trex_pv.c)."""
import os
import struct
import subprocess
import numpy as np
import pytest
from oracle import oracle, lzo_ref
from trex_amd import capi
import pv_cases
from pv_cases import W, H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = [os.path.join(ROOT, "tests", "cpp", "test_pv_read.cpp"), os.path.join(ROOT, "trex_amd", "csrc", "pvfile.cpp")]
LZO_FIX = os.path.join(ROOT, "tests", "golden", "lzo1x_streams.npz")


def _build(path, extra):
    # host only: -x c++ makes hipcc a plain C++ compiler (pv_read.h then carries no __host__ __device__)
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall"] + extra + SOURCES + ["-o", path])
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("pv_read") / "test_pv_read"), [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("pv_read_san") / "test_pv_read_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def _walk(exe, tmp_path, bodies, name="frames.bin"):
    p = tmp_path / name
    p.write_bytes(struct.pack("<I", len(bodies)) + b"".join(struct.pack("<I", len(b)) + bytes(b) for b in bodies))
    lines = _run(exe, "walk", W, H, p)
    frames, cur = [], None
    for l in lines:
        if l.startswith("frame "):
            cur = [l]
            frames.append(cur)
        else:
            cur.append(l)
    assert len(frames) == len(bodies)
    return frames


def _expected(body, blobs, runs, pixels, ts):
    """what the program prints for a good frame, from the oracle's reader and the oracle's blob records"""
    used, t, rr, pp, br, bp = oracle.pv_read_v6(body)
    assert used == len(body) and t == ts and rr.tobytes() == runs.tobytes() and pp.tobytes() == pixels.tobytes()
    out = ["frame %d ok %d %d %d %d" % (0, ts, len(br), len(rr), len(pp))]
    off, ro, po = 11, 0, 0
    for b in range(len(br)):
        q = rr[ro:ro + br[b]]
        B = blobs[b]
        box = (int(q["x0"].min()), int(q["y"].min()), int(q["x1"].max()), int(q["y"].max()))
        bid = oracle.bid(int(q[0]["x0"]), int(q[0]["x1"]), int(q[0]["y"]), int(br[b]))
        if B["n_pixels"] and B["bid"]:                                     # a record of oracle.segment: its box and bid are the reference
            assert box == (B["x0"], B["y0"], B["x1"], B["y1"]) and bid == B["bid"]
        out.append("blob %d %d %d %d %d %d %d %d %d" % ((off, int(q[0]["y"]), br[b], bp[b]) + box + (bid,)))
        out += ["line %d %d %d" % (l["x0"], l["x1"], l["y"]) for l in q]
        out.append("pixels " + bytes(pp[po:po + bp[b]]).hex())
        off += 4 + 4 * int(br[b]) + int(bp[b]); ro += int(br[b]); po += int(bp[b])
    return out


def _valid_frames():
    fr = []
    for seed in (0, 1, 2):
        b, r, px = pv_cases.scene(seed)
        fr.append((b, r, px, 123456789 + seed))
    fr.append(pv_cases.frame_tables(pv_cases.LITERAL) + (0x0102030405060708,))
    fr.append(pv_cases.frame_tables(pv_cases.TWO_BLOBS, 5) + (77,))
    e = pv_cases.scene(0)
    fr.append((e[0][:0], e[1][:0], e[2][:0], 5))                            # an empty frame: 11 bytes
    return fr


@pytest.mark.parametrize("which", ["exe", "exe_san"])
def test_walk_equals_the_oracle_reader(which, request, tmp_path):
    prog = request.getfixturevalue(which)
    frames = _valid_frames()
    bodies = [oracle.pv_serialize_v6(b, r, px, ts) for b, r, px, ts in frames]
    got = _walk(prog, tmp_path, bodies)
    for i, ((b, r, px, ts), body) in enumerate(zip(frames, bodies)):
        want = _expected(body, b, r, px, ts)
        want[0] = want[0].replace("frame 0", "frame %d" % i)
        assert got[i] == want, i


@pytest.mark.parametrize("which", ["exe", "exe_san"])
def test_every_malformed_body_is_reported(which, request, tmp_path):
    prog = request.getfixturevalue(which)
    cases = pv_cases.malformed_cases()
    assert len(cases) == 79 + 7
    got = _walk(prog, tmp_path, list(cases.values()) + [pv_cases.two_blob_body()])
    for i, name in enumerate(cases):
        assert got[i] == ["frame %d malformed" % i], name
    assert got[-1][0].startswith("frame %d ok 77 2 5 40" % len(cases))      # the body they were all made from is good


def test_the_adapter_body_writer_equals_the_oracle(exe, tmp_path):
    for k, (b, r, px, ts) in enumerate(_valid_frames()):
        txt = ["%d %d" % (ts, len(b))]
        for B in b:
            q = r[B["run_begin"]:B["run_begin"] + B["n_runs"]]
            p = px[B["pix_begin"]:B["pix_begin"] + B["n_pixels"]]
            txt.append("%d %d" % (len(q), len(p)))
            txt += ["%d %d %d" % (l["y"], l["x0"], l["x1"]) for l in q]
            txt.append(" ".join(str(int(v)) for v in p))
        (tmp_path / "frame.txt").write_text("\n".join(txt) + "\n")
        _run(exe, "serialize", tmp_path / "frame.txt", tmp_path / "frame.bin")
        assert (tmp_path / "frame.bin").read_bytes() == oracle.pv_serialize_v6(b, r, px, ts).tobytes(), k


# ---- LZO1X decoder ---------------------------------------------------------------------------------------------------------------
def _corpus():
    from test_pv_file import corpus
    return corpus()


def test_decompress_inverts_compress_and_equals_the_oracle_decoder():
    fx = np.load(LZO_FIX)
    data_all = _corpus()
    assert list(fx["sizes"]) == [len(d) for d in data_all]
    for i, data in enumerate(data_all):
        assert bytes(capi.lzo1x_decompress(capi.lzo1x_compress(data), len(data))) == data, len(data)
        for name in ("ours_%d" % i, "ref_%d" % i):                          # the recorded streams of this encoder and of the reference's
            c = fx[name].tobytes()
            want = oracle.lzo1x_decompress(c, len(data))
            assert want is not None and bytes(capi.lzo1x_decompress(c, len(data))) == bytes(want) == data, (name, len(data))
        if lzo_ref.available():
            assert bytes(capi.lzo1x_decompress(lzo_ref.compress(data), len(data))) == data


def test_decompress_refuses_a_cut_stream_and_a_short_output(exe_san, tmp_path):
    data = bytes(range(200)) * 20
    c = capi.lzo1x_compress(data)
    with pytest.raises(capi.TrexHipError) as e:
        capi.lzo1x_decompress(c[:-1], len(data))
    assert e.value.code == -1
    with pytest.raises(capi.TrexHipError) as e:
        capi.lzo1x_decompress(c, len(data) - 1)
    assert e.value.code == -1
    # the same, and a stream cut at every position, under the sanitizers: refused, never an access outside either buffer
    (tmp_path / "full.lzo").write_bytes(bytes(c))
    assert _run(exe_san, "decompress", len(data), tmp_path / "full.lzo") == ["ok %d %s" % (len(data), data.hex())]
    assert _run(exe_san, "decompress", len(data) - 1, tmp_path / "full.lzo") == ["refused"]
    small = capi.lzo1x_compress(b"abcdabcdabcdxyz" * 9)
    for k in range(len(small)):
        (tmp_path / "cut.lzo").write_bytes(bytes(small[:k]))
        assert _run(exe_san, "decompress", 135, tmp_path / "cut.lzo") == ["refused"], k


# ---- data section ------------------------------------------------------------------------------------------------------------------
def _section_frames():
    """a mix of frames below and above 15000 bytes (pv.cpp:707-708)"""
    from test_pv_file import _frames
    small, so, _ = _frames(2, False)
    big, bo, _ = _frames(2, True)
    bodies = [small[int(so[0]):int(so[1])], big[int(bo[0]):int(bo[1])], small[int(so[1]):int(so[2])], big[int(bo[1]):int(bo[2])]]
    assert [len(b) >= 15000 for b in bodies] == [False, True, False, True]
    off = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.uint64)
    return np.concatenate(bodies), off


@pytest.mark.parametrize("always_compress", [False, True])
def test_data_section_round_trip(always_compress):
    cat, off = _section_frames()
    data, idx = capi.pv_write_frames(cat, off, always_compress, file_offset=123)
    assert set(int(data[int(i) - 123]) for i in idx) == ({1} if always_compress else {0, 1})
    bodies, offsets = capi.pv_read_frames(data, idx, file_offset=123)
    assert bodies.tobytes() == cat.tobytes() and np.array_equal(offsets, off)
    # file_offset 0 through the call's own defaults
    b0, o0 = capi.pv_read_frames(*capi.pv_write_frames(cat, off, always_compress))
    assert b0.tobytes() == cat.tobytes() and np.array_equal(o0, off)
    # an index entry outside the data, a section cut short and a wrong file offset are refused
    for bad_data, bad_idx, fo in ((data, np.concatenate([idx[:-1], [123 + len(data)]]).astype(np.uint64), 123), (data[:-1], idx, 123),
                                 (data, idx, 124 + int(idx[0])), (data, idx + np.uint64(len(data)), 123)):
        with pytest.raises(capi.TrexHipError) as e:
            capi.pv_read_frames(bad_data, bad_idx, file_offset=fo)
        assert e.value.code == -1


def test_data_section_under_the_sanitizers(exe_san, tmp_path):
    cat, off = _section_frames()
    data, idx = capi.pv_write_frames(cat, off, False, file_offset=123)
    (tmp_path / "idx.bin").write_bytes(idx.tobytes())
    (tmp_path / "data.bin").write_bytes(data.tobytes())
    got = _run(exe_san, "section", 123, tmp_path / "data.bin", tmp_path / "idx.bin", 640, 480)
    heads = [l for l in got if l.startswith("frame ")]
    assert len(heads) == 4 and all(" ok " in l for l in heads), heads
    for cut in (1, 9, 200, len(data) // 2):                                  # a section cut short: refused, no read past its end
        (tmp_path / "cut.bin").write_bytes(data[:len(data) - cut].tobytes())
        assert _run(exe_san, "section", 123, tmp_path / "cut.bin", tmp_path / "idx.bin", 640, 480)[0].startswith("refused -1 "), cut
