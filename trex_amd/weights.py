"""Identity-network weights: deterministic recipe for synthetic weights + the flat blob
format libtrexhip loads (trexhip_load_weights).

Blob = little-endian: 8 x int32 header {magic 'TRXW', version 1, num_classes, width, height, channels, architecture id, 0}
(architecture id: ARCH_IDS, 0 = V118_3; the other four: shapes(arch=...), ARCH_LAYERS)
followed by float32 tensors in PyTorch state_dict order and shapes, for V118_3 those of
visual_identification_network_torch.py:184-211 (V118_3):
  conv1.weight[16,C,5,5] conv1.bias[16] bn1.weight bn1.bias bn1.running_mean bn1.running_var [16 each]
  conv2.weight[64,16,5,5] conv2.bias[64] bn2.* [64]  conv3.weight[128,64,5,5] conv3.bias[128] bn3.* [128]
  fc1.weight[100, 128*(W/8)*(H/8)] fc1.bias[100] bn4.weight[100] bn4.bias[100] (LayerNorm)
  fc2.weight[classes,100] fc2.bias[classes]
A real TRex checkpoint (<base>_dict.pth) converts with tools/convert_weights.py.
"""
import numpy as np

MAGIC = 0x57585254  # 'TRXW'

TENSORS = [
    # name, shape as function of (classes, channels, flat)
    ("conv1.weight", lambda c, ch, fl: (16, ch, 5, 5)), ("conv1.bias", lambda c, ch, fl: (16,)),
    ("bn1.weight", lambda c, ch, fl: (16,)), ("bn1.bias", lambda c, ch, fl: (16,)),
    ("bn1.running_mean", lambda c, ch, fl: (16,)), ("bn1.running_var", lambda c, ch, fl: (16,)),
    ("conv2.weight", lambda c, ch, fl: (64, 16, 5, 5)), ("conv2.bias", lambda c, ch, fl: (64,)),
    ("bn2.weight", lambda c, ch, fl: (64,)), ("bn2.bias", lambda c, ch, fl: (64,)),
    ("bn2.running_mean", lambda c, ch, fl: (64,)), ("bn2.running_var", lambda c, ch, fl: (64,)),
    ("conv3.weight", lambda c, ch, fl: (128, 64, 5, 5)), ("conv3.bias", lambda c, ch, fl: (128,)),
    ("bn3.weight", lambda c, ch, fl: (128,)), ("bn3.bias", lambda c, ch, fl: (128,)),
    ("bn3.running_mean", lambda c, ch, fl: (128,)), ("bn3.running_var", lambda c, ch, fl: (128,)),
    ("fc1.weight", lambda c, ch, fl: (100, fl)), ("fc1.bias", lambda c, ch, fl: (100,)),
    ("bn4.weight", lambda c, ch, fl: (100,)), ("bn4.bias", lambda c, ch, fl: (100,)),
    ("fc2.weight", lambda c, ch, fl: (c, 100)), ("fc2.bias", lambda c, ch, fl: (c,)),
]


# The architectures of visual_identification_network_torch.py:30-382 the library runs, by the id the blob's header word 6 carries.
# Per architecture: the convolutions (output channels, taps), BatchNorm2d or not, the flatten, fc1's width and its BatchNorm1d's name.
ARCH_IDS = {"v118_3": 0, "v100": 1, "v110": 2, "v119": 3, "v200": 4}
ARCH_NAMES = {v: k for k, v in ARCH_IDS.items()}
ARCH_LAYERS = {
    "v100": dict(convs=[(16, 5), (64, 5), (100, 5)], bn2d=False, flat=lambda w, h: 100 * (w // 8) * (h // 8), hidden=100, bn1d=None, min=8),
    "v110": dict(convs=[(16, 5), (64, 5), (100, 5)], bn2d=True, flat=lambda w, h: 100 * (w // 8) * (h // 8), hidden=100, bn1d="bn4", min=8),
    "v119": dict(convs=[(256, 5), (128, 5), (32, 5), (128, 5)], bn2d=True, flat=lambda w, h: 128 * (w // 16) * (h // 16), hidden=1024, bn1d="bn5", min=16),
    "v200": dict(convs=[(64, 3), (128, 3), (256, 3), (512, 3), (512, 3)], bn2d=True, flat=lambda w, h: 512, hidden=1024, bn1d="bn6", min=27),
}
_BN = ("weight", "bias", "running_mean", "running_var")


def arch_name(arch):
    """'v200', 'V200', 4 -> 'v200'"""
    if isinstance(arch, (int, np.integer)):
        return ARCH_NAMES[int(arch)]
    a = str(arch).lower()
    if a not in ARCH_IDS:
        raise ValueError(f"unknown identity network version {arch!r}: one of {sorted(ARCH_IDS)}")
    return a


def shapes(num_classes, channels=1, width=80, height=80, arch="v118_3"):
    """(name, shape) of every tensor in the architecture's state_dict order, without num_batches_tracked"""
    arch = arch_name(arch)
    if arch == "v118_3":
        flat = 128 * (width // 8) * (height // 8)
        return [(n, f(num_classes, channels, flat)) for n, f in TENSORS]
    L = ARCH_LAYERS[arch]
    out, ci = [], channels
    for i, (co, k) in enumerate(L["convs"], 1):
        out += [(f"conv{i}.weight", (co, ci, k, k)), (f"conv{i}.bias", (co,))]
        if L["bn2d"]:
            out += [(f"bn{i}.{t}", (co,)) for t in _BN]
        ci = co
    hid = L["hidden"]
    out += [("fc1.weight", (hid, L["flat"](width, height))), ("fc1.bias", (hid,))]
    if L["bn1d"]:
        out += [(f"{L['bn1d']}.{t}", (hid,)) for t in _BN]
    out += [("fc2.weight", (num_classes, hid)), ("fc2.bias", (num_classes,))]
    return out


def synthetic_state(num_classes, seed, channels=1, width=80, height=80, arch="v118_3"):
    """Deterministic random weights (numpy PCG64, reproducible anywhere numpy runs): uniform
    +-1/sqrt(fan_in) like PyTorch's default init, non-trivial BN/LayerNorm affine.  Running
    statistics are placeholders here; calibrated values come from the golden fixture."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, shp in shapes(num_classes, channels, width, height, arch):
        if name.endswith("running_mean"):
            st[name] = np.zeros(shp, np.float32)
        elif name.endswith("running_var"):
            st[name] = np.ones(shp, np.float32)
        elif name.startswith("bn") and name.endswith("weight"):
            st[name] = rng.uniform(0.5, 1.5, shp).astype(np.float32)
        elif name.startswith("bn") and name.endswith("bias"):
            st[name] = rng.uniform(-0.3, 0.3, shp).astype(np.float32)
        else:
            fan_in = int(np.prod(shp[1:])) if len(shp) > 1 else None
            if fan_in is None:   # bias of the preceding layer
                prev = st[name.replace("bias", "weight")]
                fan_in = int(np.prod(prev.shape[1:]))
            b = 1.0 / np.sqrt(fan_in)
            st[name] = rng.uniform(-b, b, shp).astype(np.float32)
    st["fc2.weight"] = (st["fc2.weight"] * 8.0).astype(np.float32)   # peaky softmax: a flat one hides errors
    return st


def synthetic_crops(n, seed, channels=1, width=80, height=80):
    """uint8 NHWC crops that look like blobs on black: a bright ellipse with texture."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    out = np.zeros((n, height, width, channels), np.uint8)
    for i in range(n):
        a, b = rng.uniform(12, 30), rng.uniform(4, 10)
        th = rng.uniform(0, np.pi)
        u = (xx - width / 2) * np.cos(th) + (yy - height / 2) * np.sin(th)
        v = -(xx - width / 2) * np.sin(th) + (yy - height / 2) * np.cos(th)
        m = (u / a) ** 2 + (v / b) ** 2 <= 1
        tex = rng.integers(40, 200, (height, width, channels))
        out[i][m] = tex[m]
    return out


def pack_blob(state, num_classes, channels=1, width=80, height=80, arch="v118_3"):
    hdr = np.array([MAGIC, 1, num_classes, width, height, channels, ARCH_IDS[arch_name(arch)], 0], np.int32)
    parts = [hdr.tobytes()]
    for name, shp in shapes(num_classes, channels, width, height, arch):
        t = np.ascontiguousarray(state[name], np.float32)
        assert t.shape == tuple(shp), (name, t.shape, shp)
        parts.append(t.tobytes())
    return b"".join(parts)


def blob_arch(blob):
    """the architecture name a blob's header word 6 names"""
    return arch_name(int(np.frombuffer(blob[24:28], np.int32)[0]))


def unpack_blob(blob, arch="v118_3"):
    """Inverse of pack_blob: -> (state dict, num_classes, channels).  `arch` must be the blob's own (blob_arch)."""
    hdr = np.frombuffer(blob[:32], np.int32)
    assert int(hdr[0]) == MAGIC and int(hdr[1]) == 1, "not a TRXW v1 blob"
    classes, width, height, channels = int(hdr[2]), int(hdr[3]), int(hdr[4]), int(hdr[5])
    assert int(hdr[6]) == ARCH_IDS[arch_name(arch)], f"the blob holds {ARCH_NAMES.get(int(hdr[6]), int(hdr[6]))}, not {arch}"
    st, off = {}, 32
    for name, shp in shapes(classes, channels, width, height, arch):
        cnt = int(np.prod(shp))
        st[name] = np.frombuffer(blob[off:off + 4 * cnt], np.float32).reshape(shp).copy()
        off += 4 * cnt
    assert off == len(blob), "blob size does not match its header"
    return st, classes, channels


def synthetic_train_batch(n, seed, classes, channels=1):
    """Training inputs as TRexImageDataset hands them over (visual_recognition_torch.py:158-188): NHWC float32 in [0, 255],
    NOT integer (the augmentation rescales), + integer class labels."""
    rng = np.random.default_rng(seed)
    x = synthetic_crops(n, seed + 7, channels).astype(np.float32)
    x = np.clip(x * rng.uniform(0.85, 1.15, (n, 1, 1, 1)).astype(np.float32) + rng.uniform(0.0, 3.0, x.shape).astype(np.float32) * (x > 0), 0.0, 255.0)
    y = rng.integers(0, classes, n).astype(np.int32)
    return np.ascontiguousarray(x, np.float32), y


# ---- the category network (trex_learn_category.py:18-44, PyTorchModel) ----
# Its blob: 8 x int32 header {magic 'TRXC', version 1, categories, width, height, channels, 0, 0}, then the float32 tensors in the module's
# state_dict order (declaration order: the three convolutions, the three BatchNorm2d, fc1, fc2), without num_batches_tracked.  The magic differs
# from an identity blob's, so trexhip_load_weights refuses it and trexhip_categorize_load_weights refuses an identity blob; ARCH_IDS has no entry
# for it.  A checkpoint's 'model_state' converts with tools/convert_category_weights.py.
CATEGORY_MAGIC = 0x43585254  # 'TRXC'
CATEGORY_CONVS = (16, 64, 100)


def category_shapes(categories, channels=1, width=80, height=80):
    """(name, shape) of every tensor of the category network in its state_dict order"""
    out, ci = [], channels
    for i, co in enumerate(CATEGORY_CONVS, 1):
        out += [(f"conv{i}.weight", (co, ci, 3, 3)), (f"conv{i}.bias", (co,))]
        ci = co
    for i, co in enumerate(CATEGORY_CONVS, 1):
        out += [(f"batch_norm{i}.{t}", (co,)) for t in _BN]
    out += [("fc1.weight", (100, 100 * (width // 8) * (height // 8))), ("fc1.bias", (100,)), ("fc2.weight", (categories, 100)), ("fc2.bias", (categories,))]
    return out


def synthetic_category_state(categories, seed, channels=1, width=80, height=80):
    """The recipe of synthetic_state for the category network; every third BatchNorm2d scale is negative (the BatchNorm stands in front of the
    max-pool: a negative scale makes the pool pick what was the window's minimum)."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, shp in category_shapes(categories, channels, width, height):
        if name.endswith("running_mean"):
            st[name] = np.zeros(shp, np.float32)
        elif name.endswith("running_var"):
            st[name] = np.ones(shp, np.float32)
        elif name.startswith("batch_norm") and name.endswith("weight"):
            g = rng.uniform(0.5, 1.5, shp).astype(np.float32)
            g[::3] = -g[::3]
            st[name] = g
        elif name.startswith("batch_norm") and name.endswith("bias"):
            st[name] = rng.uniform(-0.3, 0.3, shp).astype(np.float32)
        else:
            fan_in = int(np.prod(shp[1:])) if len(shp) > 1 else int(np.prod(st[name.replace("bias", "weight")].shape[1:]))
            b = 1.0 / np.sqrt(fan_in)
            st[name] = rng.uniform(-b, b, shp).astype(np.float32)
    st["fc2.weight"] = (st["fc2.weight"] * 8.0).astype(np.float32)   # peaky softmax: a flat one hides errors
    return st


def pack_category_blob(state, categories, channels=1, width=80, height=80):
    hdr = np.array([CATEGORY_MAGIC, 1, categories, width, height, channels, 0, 0], np.int32)
    parts = [hdr.tobytes()]
    for name, shp in category_shapes(categories, channels, width, height):
        if name not in state:
            raise ValueError(f"{name} is missing")
        t = np.ascontiguousarray(state[name], np.float32)
        if t.shape != tuple(shp):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, the category network of {categories} categories at {width}x{height}x{channels} has {tuple(shp)}")
        parts.append(t.tobytes())
    return b"".join(parts)


def unpack_category_blob(blob):
    """Inverse of pack_category_blob: -> (state dict, categories, channels, width, height)"""
    hdr = np.frombuffer(blob[:32], np.int32)
    assert int(hdr[0]) == CATEGORY_MAGIC and int(hdr[1]) == 1, "not a TRXC v1 blob"
    categories, width, height, channels = int(hdr[2]), int(hdr[3]), int(hdr[4]), int(hdr[5])
    st, off = {}, 32
    for name, shp in category_shapes(categories, channels, width, height):
        cnt = int(np.prod(shp))
        st[name] = np.frombuffer(blob[off:off + 4 * cnt], np.float32).reshape(shp).copy()
        off += 4 * cnt
    assert off == len(blob), "blob size does not match its header"
    return st, categories, channels, width, height
