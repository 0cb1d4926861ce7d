#!/usr/bin/env python3
"""Convert a TRex categorisation checkpoint into the flat blob trexhip_categorize_load_weights() takes.

The reference saves {'model_state': state_dict, 'optimizer_state', 'samples', 'labels', 'validation_indexes', 'categories_map', 'categories'}
(trex_learn_category.py:343-351); only 'model_state' is read.  Its tensors are those of PyTorchModel (:18-44): three 3x3 convolutions, three
BatchNorm2d, fc1 and fc2.  The crop size cannot be read off the tensors alone (fc1 only knows (W // 8) * (H // 8)), so width and height are arguments;
channels and categories come from conv1.weight and fc2.weight.

    python tools/convert_category_weights.py categories.pth categories.trxc --width 80 --height 80

The way back -- a blob that trexhip_trainer_export wrote, as a checkpoint holding {'model_state': state_dict} that PyTorchModel.load_state_dict
takes (the blob knows its own size; num_batches_tracked is not a weight and is left to the module's default):

    python tools/convert_category_weights.py --from-blob categories.trxc categories.pth
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trex_amd import weights  # noqa: E402


def convert(obj, width, height):
    """checkpoint object (as torch.load returns it) -> (blob bytes, categories, channels).  ValueError names the tensor that is missing or has
    another shape than the category network's at width x height."""
    if not isinstance(obj, dict) or "model_state" not in obj:
        raise ValueError("not a categorisation checkpoint: a dict with 'model_state' is expected (trex_learn_category.py:343-351)")
    sd = obj["model_state"]
    clean = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}      # BatchNorm's step counter is not a weight
    for name in ("conv1.weight", "fc2.weight"):
        if name not in clean:
            raise ValueError(f"{name} is missing from model_state")
    shape = lambda t: tuple(int(x) for x in t.shape)
    if len(shape(clean["conv1.weight"])) != 4 or len(shape(clean["fc2.weight"])) != 2:
        raise ValueError(f"conv1.weight / fc2.weight have shapes {shape(clean['conv1.weight'])} / {shape(clean['fc2.weight'])}: not the category network's")
    channels, categories = shape(clean["conv1.weight"])[1], shape(clean["fc2.weight"])[0]
    want = weights.category_shapes(categories, channels, width, height)
    st = {}
    for name, shp in want:
        if name not in clean:
            raise ValueError(f"{name} is missing from model_state")
        t = clean[name]
        t = t.detach().cpu().float().numpy() if hasattr(t, "detach") else t
        if shape(t) != tuple(shp):
            raise ValueError(f"{name} has shape {shape(t)}, the category network of {categories} categories at {width}x{height}x{channels} has {tuple(shp)}")
        st[name] = t
    extra = sorted(set(clean) - {n for n, _ in want})
    if extra:
        raise ValueError(f"model_state holds tensors the category network does not have: {extra[:6]}")
    return weights.pack_category_blob(st, categories, channels, width, height), categories, channels


def model_state(blob):
    """'TRXC' blob -> the module's state_dict as torch tensors, in its declaration order"""
    import torch
    st, categories, channels, width, height = weights.unpack_category_blob(blob)
    return {k: torch.from_numpy(v) for k, v in st.items()}, categories, channels, width, height


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("output")
    ap.add_argument("--width", type=int, default=80, help="individual_image_size, width")
    ap.add_argument("--height", type=int, default=80, help="individual_image_size, height")
    ap.add_argument("--from-blob", action="store_true", help="the way back: `checkpoint` is a 'TRXC' blob, `output` the checkpoint to write")
    a = ap.parse_args()
    import torch
    if a.from_blob:
        with open(a.checkpoint, "rb") as f:
            sd, categories, channels, width, height = model_state(f.read())
        torch.save({"model_state": sd}, a.output)
        print(f"{a.output}: model_state of {categories} categories, {width}x{height}x{channels}")
        return
    obj = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    blob, categories, channels = convert(obj, a.width, a.height)
    with open(a.output, "wb") as f:
        f.write(blob)
    print(f"{a.output}: {len(blob)} bytes, {categories} categories, {a.width}x{a.height}x{channels}")


if __name__ == "__main__":
    main()
