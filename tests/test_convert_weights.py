"""tools/convert_weights.py on a checkpoint laid out like the reference writes it (visual_recognition_torch.py:102-117:
{'model': None, 'state_dict': ..., 'metadata': {'input_shape': (W,H,C), 'num_classes', 'model_type', ...}}, keys with the
PermuteAxesWrapper 'model.' prefix and BatchNorm's num_batches_tracked) -- round trip into the blob trexhip_load_weights takes."""
import importlib.util
import os
import numpy as np
import pytest
import torch
from trex_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("convert_weights", os.path.join(ROOT, "tools", "convert_weights.py"))
cw = importlib.util.module_from_spec(spec); spec.loader.exec_module(cw)


def reference_style_checkpoint(classes, channels):
    st = weights.synthetic_state(classes, 7, channels=channels)
    sd = {"model." + k: torch.from_numpy(v) for k, v in st.items()}
    for i in (1, 2, 3):
        sd[f"model.bn{i}.num_batches_tracked"] = torch.tensor(12345)
    ck = {"model": None, "state_dict": sd,
          "metadata": {"input_shape": (80, 80, channels), "num_classes": classes, "video_name": "x", "epoch": 3, "uniqueness": 0.9, "model_type": "v118_3"}}
    return st, ck


@pytest.mark.parametrize("classes,channels", [(8, 1), (100, 3)])
def test_round_trip(tmp_path, classes, channels):
    st, ck = reference_style_checkpoint(classes, channels)
    path = tmp_path / "model_dict.pth"
    torch.save(ck, path)
    obj = torch.load(path, map_location="cpu", weights_only=False)
    blob, c, w, h, ch = cw.convert(obj)
    assert (c, w, h, ch) == (classes, 80, 80, channels)
    assert blob == weights.pack_blob(st, classes, channels)
    # a bare state_dict (no wrapper, no prefix) converts to the same blob
    blob2, *_ = cw.convert({k: torch.from_numpy(v) for k, v in st.items()})
    assert blob2 == blob


def test_rejects_other_networks_and_bad_shapes():
    st, ck = reference_style_checkpoint(8, 1)
    ck["metadata"]["model_type"] = "v200"
    with pytest.raises(ValueError):
        cw.convert(ck)
    st, ck = reference_style_checkpoint(8, 1)
    ck["state_dict"]["model.fc1.weight"] = torch.zeros(100, 7)
    with pytest.raises(ValueError):
        cw.convert(ck)
    st, ck = reference_style_checkpoint(8, 1)
    del ck["state_dict"]["model.bn4.bias"]
    with pytest.raises(KeyError):
        cw.convert(ck)


def test_arbitrary_bit_patterns_survive_blob_and_converter():
    """what a TRAINED network holds -- any float32 whatsoever: denormals, huge and tiny magnitudes, negative zero -- goes through pack_blob,
    unpack_blob and the converter bit for bit (the values above are uniform(+-1/sqrt(fan_in)): one exponent range).  The device-trained state
    itself takes the same trip in tests/test_cnn_trained_gpu.py."""
    rng = np.random.default_rng(3)
    st = {}
    for name, shp in weights.shapes(16):
        bits = rng.integers(0, 1 << 32, int(np.prod(shp)), dtype=np.uint64).astype(np.uint32)
        bits[(bits & 0x7f800000) == 0x7f800000] &= 0x807fffff            # no inf / NaN: NaN payloads need not survive a torch tensor
        st[name] = bits.view(np.float32).reshape(shp)
    st["fc2.bias"][:3] = [-0.0, np.float32(1e-45), np.float32(-3e38)]
    blob = weights.pack_blob(st, 16)
    back, classes, channels = weights.unpack_blob(blob)
    assert (classes, channels) == (16, 1)
    for k in st:
        assert back[k].tobytes() == st[k].tobytes(), k
    assert weights.pack_blob(back, 16) == blob
    blob2, c, w, h, ch = cw.convert({"model." + k: torch.from_numpy(v.copy()) for k, v in st.items()})
    assert (c, w, h, ch) == (16, 80, 80, 1) and blob2 == blob
