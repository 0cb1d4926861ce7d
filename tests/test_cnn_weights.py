"""The identity network's weight preparation (trex_amd/csrc/cnn_weights.h) on the CPU: tests/cpp/test_cnn_weights.cpp runs the blob parser and
every packer, and each operand image is compared byte for byte with a numpy restatement written from the layout comments of that header.
The BatchNorm fold is float64 rounded once to float32 on both sides, fp16 pieces are np.float16 casts, bf16 pieces the integer
round-to-nearest-even formula."""
import math
import os
import subprocess
import numpy as np
import pytest
from trex_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CLASSES = 7
CASES = [(1, 80, 80), (3, 80, 80), (3, 96, 40)]          # (CH, W, H)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_weights") / "test_cnn_weights")
    # host only: -x c++ makes hipcc a C++ compiler that knows _Float16 (the packers' fp16 rounding)
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "trex_amd", "csrc", "cnn_weights.hip"),
                           os.path.join(ROOT, "tests", "cpp", "test_cnn_weights.cpp"), "-o", path])
    return path


def run(exe, blob, tmp_path):
    out = tmp_path / "images"
    out.mkdir(exist_ok=True)
    (tmp_path / "blob.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "blob.bin"), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines(), out


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def fold(st, conv, bn):
    """conv weight [CO][CI][5][5] and bias with the eval-mode BatchNorm folded in, in float64, rounded once"""
    s = st[bn + ".weight"].astype(np.float64) / np.sqrt(st[bn + ".running_var"].astype(np.float64) + 1e-5)
    b = (st[conv + ".bias"].astype(np.float64) - st[bn + ".running_mean"].astype(np.float64)) * s + st[bn + ".bias"].astype(np.float64)
    return (st[conv + ".weight"].astype(np.float64) * s[:, None, None, None]).astype(np.float32), b.astype(np.float32)


def chunked(w, cic):
    """[CO][CI][5][5] -> [CI/CIC][25][CIC][CO]"""
    co, ci = w.shape[:2]
    return np.ascontiguousarray(w.reshape(co, ci // cic, cic, 25).transpose(1, 3, 2, 0))


def scale_of(max_abs):
    k = 0
    if max_abs > 0:
        k = min(24, max(-24, math.floor(math.log2(16384.0 / float(max_abs)))))
    return k


def bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_pieces(x):
    back = lambda p: (p.astype(np.uint32) << np.uint32(16)).view(np.float32)
    p1 = bf16(x)
    r1 = x - back(p1)
    p2 = bf16(r1)
    return np.stack([p1, p2, bf16(r1 - back(p2))])


def f16_pieces(x):
    x = np.ascontiguousarray(x, np.float32)
    h1 = x.astype(np.float16)
    h2 = (x - h1.astype(np.float32)).astype(np.float16)
    return np.stack([h1, h2]).view(np.uint16)


def mfma_order(pieces):
    """pieces [piece][cc][t][k][co] -> [cc][t][piece][k/8][co][8]"""
    n, ncc, t, k, co = pieces.shape
    return np.ascontiguousarray(pieces.reshape(n, ncc, t, k // 8, 8, co).transpose(1, 2, 0, 3, 5, 4))


def f16_image(packed):
    k = scale_of(np.abs(packed).max())
    return mfma_order(f16_pieces(packed * np.float32(2.0 ** k))), k


G = np.array([[-1, 0, 0, 0, 0],
              [-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9],
              [-2.0 / 9, 2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9],
              [1.0 / 90, 1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45],
              [1.0 / 90, -1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45],
              [32.0 / 45, 16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45],
              [32.0 / 45, -16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45],
              [0, 0, 0, 0, 1]], np.float64)


def wino_image(packed):
    """Wt[ky][p] = sum over kx of G[p][kx] w[ky][kx] in float64 (kx ascending), [cc][ky * 8 + p][16][CO]; then as the fp16 image"""
    ncc, _, cic, co = packed.shape
    w = packed.reshape(ncc, 5, 5, cic, co).astype(np.float64)
    wt = np.zeros((ncc, 5, 8, cic, co), np.float64)
    for kx in range(5):
        wt = wt + G[:, kx][None, None, :, None, None] * w[:, :, kx][:, :, None]
    wt = wt.reshape(ncc, 40, cic, co)
    k = scale_of(np.abs(wt).max())
    return mfma_order(f16_pieces((wt * 2.0 ** k).astype(np.float32))), k


def conv1_frags(w1, ch):
    """[shift s][mfma m 0..CH][piece][lane = q * 16 + co][slot]: slot j = tap kx = j - s; m < CH: channel m, row ky = q; m == CH: row 4 of channel q"""
    k = scale_of(np.abs(w1).max())
    rows = (w1 * np.float32(2.0 ** k)).reshape(ch, 5, 5, 16)            # [ch][ky][kx][co]
    t = np.zeros((4, ch + 1, 4, 16, 8), np.float32)                      # [s][m][q][co][slot]
    for s in range(4):
        t[s, :ch, :, :, s:s + 5] = rows[:, :4].transpose(0, 1, 3, 2)
        t[s, ch, :ch, :, s:s + 5] = rows[:, 4].transpose(0, 2, 1)
    return np.ascontiguousarray(f16_pieces(t).transpose(1, 2, 0, 3, 4, 5)), k


def expected(st, ch, w, h):
    e, inv = {}, {}
    c1w, e["c1_b"] = fold(st, "conv1", "bn1")
    e["c1_w"] = np.ascontiguousarray(c1w.reshape(16, ch, 25).transpose(1, 2, 0))
    e["c1_frags"], inv["c1_frags"] = conv1_frags(e["c1_w"], ch)
    for name, conv, bn in (("c2", "conv2", "bn2"), ("c3", "conv3", "bn3")):
        wf, e[name + "_b"] = fold(st, conv, bn)
        e[name + "_w"] = chunked(wf, 16)
        e[name + "_bf16"] = mfma_order(bf16_pieces(e[name + "_w"]))
        e[name + "_f16"], inv[name + "_f16"] = f16_image(e[name + "_w"])
        e[name + "_wino"], inv[name + "_wino"] = wino_image(e[name + "_w"])
    e["c3x32_w"], e["c3x32_b"] = chunked(wf, 32), e["c3_b"]
    p = (w // 8) * (h // 8)
    e["fc1_w"] = np.zeros((p, 128, 128), np.float32)                     # [h * (W/8) + w][c][o padded to 128]
    e["fc1_w"][:, :, :100] = st["fc1.weight"].reshape(100, 128, p).transpose(2, 1, 0)
    e["fc1_b"] = np.zeros(128, np.float32)
    e["fc1_b"][:100] = st["fc1.bias"]
    k = scale_of(np.abs(e["fc1_w"]).max())
    inv["fc1_f16"] = k                                                   # [K/8][piece][128][8]
    e["fc1_f16"] = np.ascontiguousarray(f16_pieces(e["fc1_w"].reshape(p * 16, 8, 128) * np.float32(2.0 ** k)).transpose(1, 0, 3, 2))
    e["fc2_t"] = np.ascontiguousarray(st["fc2.weight"].T)
    return e, inv


@pytest.mark.parametrize("ch,w,h", CASES)
def test_every_image_byte_for_byte(exe, tmp_path, ch, w, h):
    st = weights.synthetic_state(CLASSES, 31 + ch + w, ch, w, h)
    for bn in ("bn1", "bn2", "bn3"):                                     # running statistics that make the fold do something
        rng = np.random.default_rng(len(st[bn + ".bias"]))
        st[bn + ".running_mean"] = rng.uniform(-0.2, 0.2, st[bn + ".bias"].shape).astype(np.float32)
        st[bn + ".running_var"] = rng.uniform(0.5, 2.0, st[bn + ".bias"].shape).astype(np.float32)
    lines, out = run(exe, weights.pack_blob(st, CLASSES, ch, w, h), tmp_path)
    assert lines[0] == f"header {CLASSES} {w} {h} {ch}", lines
    want, want_k = expected(st, ch, w, h)
    got_inv = {l.split()[1]: float.fromhex(l.split()[2]) for l in lines if l.startswith("inv ")}
    assert got_inv == {name: 2.0 ** -k for name, k in want_k.items()}
    assert sorted(os.listdir(out)) == sorted(name + ".bin" for name in want)
    for name, a in want.items():
        got = (out / (name + ".bin")).read_bytes()
        assert got == a.tobytes(), f"{name}: {len(got)} bytes against {a.nbytes}" + (
            f", first difference at byte {int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(a.tobytes(), np.uint8))[0])}"
            if len(got) == a.nbytes else "")


def test_the_parser_refuses_what_it_refused(exe, tmp_path):
    good = weights.pack_blob(weights.synthetic_state(CLASSES, 5), CLASSES)

    def header(**kw):
        hdr = np.frombuffer(good[:32], np.int32).copy()
        for field, v in kw.items():
            hdr[{"magic": 0, "version": 1, "classes": 2, "channels": 5}[field]] = v
        return hdr.tobytes() + good[32:]

    E_INVALID, E_UNSUPPORTED = -1, -4
    for blob, code, text in ((good[:31], E_INVALID, "blob too small"),
                             (header(magic=0x57585255), E_INVALID, "bad magic/version"),
                             (header(version=2), E_INVALID, "bad magic/version"),
                             (good + b"\0\0\0\0", E_INVALID, "blob size does not match its header"),
                             (good[:-4], E_INVALID, "blob size does not match its header"),
                             (header(channels=2), E_UNSUPPORTED, "channels must be 1 or 3"),
                             (header(classes=0), E_INVALID, "classes must be 1..1024"),
                             (header(classes=1025), E_INVALID, "classes must be 1..1024")):
        lines, _ = run(exe, blob, tmp_path)
        assert lines == [f"refused {code} trexhip_load_weights: {text}"], lines
