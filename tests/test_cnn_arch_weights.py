"""The weight preparation of the identity networks v100 / v110 / v119 / v200 (trex_amd/csrc/cnn_weights.h) on the CPU:
tests/cpp/test_cnn_arch_weights.cpp runs parse_arch_blob and every packer the way the loader calls them, and each operand image is compared
byte for byte with a numpy restatement written from the layout comments of that header.  The BatchNorm fold is float64 rounded once to
float32 on both sides, fp16 pieces are np.float16 casts, bf16 pieces the integer round-to-nearest-even formula (test_cnn_weights.py)."""
import os
import subprocess
import numpy as np
import pytest
from trex_amd import weights
from test_cnn_weights import bf16_pieces, f16_pieces, scale_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CLASSES = 7
CASES = [("v100", 1, 16, 24), ("v110", 3, 24, 16), ("v119", 1, 32, 16), ("v200", 3, 27, 30)]          # (arch, CH, W, H)
E_INVALID, E_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cnn_arch_weights") / "test_cnn_arch_weights")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "trex_amd", "csrc", "cnn_weights.hip"),
                           os.path.join(ROOT, "tests", "cpp", "test_cnn_arch_weights.cpp"), "-o", path])
    return path


def run(exe, blob, tmp_path):
    out = tmp_path / "images"
    out.mkdir(exist_ok=True)
    (tmp_path / "blob.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "blob.bin"), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines(), out


def pad(c):
    return 16 if c <= 16 else (c + 31) // 32 * 32


def pieces_image(pieces):
    """pieces [piece][tile][k = 16][co] -> [tile][piece][k/8][co][8]"""
    n, tiles, k, co = pieces.shape
    return np.ascontiguousarray(pieces.reshape(n, tiles, k // 8, 8, co).transpose(1, 0, 2, 4, 3))


def expected(st, arch, ch, w, h):
    L = weights.ARCH_LAYERS[arch]
    fold = L["bn2d"] and arch != "v110"
    e, inv = {}, {}
    ci, ci_pad = ch, ch
    for i, (co, t) in enumerate(L["convs"], 1):
        n = f"c{i}"
        co_pad = pad(co)
        wt, b = st[f"conv{i}.weight"].astype(np.float64), st[f"conv{i}.bias"]
        s = np.ones(co)
        if L["bn2d"]:
            s = st[f"bn{i}.weight"].astype(np.float64) / np.sqrt(st[f"bn{i}.running_var"].astype(np.float64) + 1e-5)
        bias, sv, tv = np.zeros(co_pad, np.float32), np.zeros(co_pad, np.float32), np.zeros(co_pad, np.float32)
        if fold:
            wt = wt * s[:, None, None, None]
            bias[:co] = ((b.astype(np.float64) - st[f"bn{i}.running_mean"].astype(np.float64)) * s + st[f"bn{i}.bias"].astype(np.float64)).astype(np.float32)
            sv[:co] = 1
        else:
            bias[:co] = b
            sv[:co] = s.astype(np.float32)
            if L["bn2d"]:
                tv[:co] = (st[f"bn{i}.bias"].astype(np.float64) - st[f"bn{i}.running_mean"].astype(np.float64) * s).astype(np.float32)
        full = np.zeros((co_pad, ci_pad, t * t), np.float32)
        full[:co, :ci] = wt.astype(np.float32).reshape(co, ci, t * t)
        if i == 1:       # [CO_pad/16][CH][T*T][16]
            e[n + "_w"] = np.ascontiguousarray(full.reshape(co_pad // 16, 16, ch, t * t).transpose(0, 2, 3, 1))
        else:            # [CO_pad/COB][CI_pad/16][T*T][16][COB]
            cob = min(co_pad, 128)
            img = np.ascontiguousarray(full.reshape(co_pad // cob, cob, ci_pad // 16, 16, t * t).transpose(0, 2, 4, 3, 1))
            e[n + "_w"] = img
            tiles = img.reshape(-1, 16, cob)
            e[n + "_bf16"] = pieces_image(bf16_pieces(tiles))
            k = scale_of(np.abs(tiles).max())
            inv[n + "_f16"] = k
            e[n + "_f16"] = pieces_image(f16_pieces(tiles * np.float32(2.0 ** k)))
        e[n + "_b"], e[n + "_s"], e[n + "_t"] = bias, sv, tv
        ci, ci_pad = co, co_pad
        if arch == "v200":
            if i in (2, 4, 5):
                w, h = w // 3, h // 3
        else:
            w, h = w // 2, h // 2
    hid = L["hidden"]
    nh = pad(hid)
    p = 1 if arch == "v200" else w * h
    e["fc1_w"] = np.zeros((p, ci_pad, nh), np.float32)                   # [hw][c padded][o padded]
    e["fc1_w"][:, :ci, :hid] = st["fc1.weight"].reshape(hid, ci, p).transpose(2, 1, 0)
    e["fc1_b"] = np.zeros(nh, np.float32)
    e["fc1_b"][:hid] = st["fc1.bias"]
    e["head_s"], e["head_t"] = np.zeros(nh, np.float32), np.zeros(nh, np.float32)
    e["head_s"][:hid] = 1
    if L["bn1d"]:
        bn = L["bn1d"]
        s = st[bn + ".weight"].astype(np.float64) / np.sqrt(st[bn + ".running_var"].astype(np.float64) + 1e-5)
        e["head_s"][:hid] = s.astype(np.float32)
        e["head_t"][:hid] = (st[bn + ".bias"].astype(np.float64) - st[bn + ".running_mean"].astype(np.float64) * s).astype(np.float32)
    e["fc2_t"] = np.ascontiguousarray(st["fc2.weight"].T)
    return e, inv


@pytest.mark.parametrize("arch,ch,w,h", CASES)
def test_every_image_byte_for_byte(exe, tmp_path, arch, ch, w, h):
    st = weights.synthetic_state(CLASSES, 41 + ch + w, ch, w, h, arch=arch)
    for k in st:                                                         # running statistics that make the fold do something
        rng = np.random.default_rng(len(st[k]) + len(k))
        if k.endswith("running_mean"):
            st[k] = rng.uniform(-0.2, 0.2, st[k].shape).astype(np.float32)
        if k.endswith("running_var"):
            st[k] = rng.uniform(0.5, 2.0, st[k].shape).astype(np.float32)
    blob = weights.pack_blob(st, CLASSES, ch, w, h, arch=arch)
    lines, out = run(exe, blob, tmp_path)
    aid = weights.ARCH_IDS[arch]
    assert lines[0] == f"v118_3 {E_UNSUPPORTED} trexhip_trainer_create: the blob holds a {arch} network; only v118_3 is implemented here", lines
    assert lines[1] == f"header {aid} {CLASSES} {w} {h} {ch} id {aid} bytes {len(blob)}", lines
    want, want_k = expected(st, arch, ch, w, h)
    got_inv = {l.split()[1]: float.fromhex(l.split()[2]) for l in lines if l.startswith("inv ")}
    assert got_inv == {name: 2.0 ** -k for name, k in want_k.items()}
    assert sorted(os.listdir(out)) == sorted(name + ".bin" for name in want)
    for name, a in want.items():
        got = (out / (name + ".bin")).read_bytes()
        assert got == a.tobytes(), f"{name}: {len(got)} bytes against {a.nbytes}" + (
            f", first difference at byte {int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(a.tobytes(), np.uint8))[0])}"
            if len(got) == a.nbytes else "")


def test_the_parsers_refuse(exe, tmp_path):
    good = weights.pack_blob(weights.synthetic_state(CLASSES, 5, 1, 27, 27, arch="v200"), CLASSES, 1, 27, 27, arch="v200")

    def header(**kw):
        hdr = np.frombuffer(good[:32], np.int32).copy()
        for field, v in kw.items():
            hdr[{"classes": 2, "width": 3, "height": 4, "channels": 5, "arch": 6}[field]] = v
        return hdr.tobytes() + good[32:]

    for blob, code, text in ((header(width=26), E_UNSUPPORTED, "individual_image_size 26x27 is outside 27..256 x 27..256, the range of v200 (minimum 27)"),
                             (header(arch=3, width=15, height=16), E_UNSUPPORTED, "individual_image_size 15x16 is outside 16..256 x 16..256, the range of v119 (minimum 16)"),
                             (header(arch=5), E_INVALID, "unknown network version id 5 (0..4: v118_3, v100, v110, v119, v200)"),
                             (header(arch=-1), E_INVALID, "unknown network version id -1 (0..4: v118_3, v100, v110, v119, v200)"),
                             (header(arch=3), E_INVALID, "blob size does not match its header (v119)"),
                             (good[:-4], E_INVALID, "blob size does not match its header (v200)"),
                             (header(channels=2), E_UNSUPPORTED, "channels must be 1 or 3"),
                             (header(classes=1025), E_INVALID, "classes must be 1..1024")):
        lines, _ = run(exe, blob, tmp_path)
        assert lines[1] == f"refused {code} trexhip_load_weights: {text}", lines
    # the trainer's parser: an id outside 0..4 is invalid, another architecture unsupported, and word 6 == 0 is what it always was
    assert run(exe, header(arch=5), tmp_path)[0][0] == f"v118_3 {E_INVALID} trexhip_trainer_create: unknown network version id 5 (0..4: v118_3, v100, v110, v119, v200)"
    old = weights.pack_blob(weights.synthetic_state(CLASSES, 5), CLASSES)
    assert run(exe, old, tmp_path)[0][0] == "v118_3 0 "
