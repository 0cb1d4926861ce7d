"""Generates tests/golden/cnn_trained_stats.npz by TRAINING the reference's own network module
(/root/reference/Application/src/tracker/python/visual_identification_network_torch.py, V118_3 behind PermuteAxesWrapper, imported the
way make_train_fixture.py does) with torch.optim.Adam(lr 1e-3) + nn.CrossEntropyLoss + ReduceLROnPlateau(min, 0.1, patience 5) on exactly
the stream tests/trained_net.py feeds the device trainer: tests/identity_synth.py, same start weights, same batches, same epochs, the
module's own dropout draws.  Three dropout seeds: their spread is the yardstick for a run that draws other masks.

  python tests/golden/make_trained_stats_fixture.py          (about a quarter of an hour on 8 cores)

Stored: numbers only, a few KB -- per seed and epoch the training loss, validation loss and accuracy; per seed the float64 oracle's test
accuracy and mean top softmax on the trained weights, and the 50 / 99 / 100 % quantiles of oracle.cnn_oracle.stage_maxima over the test
set.  No weights and nothing of the reference's text.  The generator asserts what the tests rely on: every run is "trained" (>= 95 % test
accuracy, mean top softmax >= 0.9) and its training loss falls from epoch to epoch over the first MONO_EPOCHS epochs.
"""
import os
import sys
import time
import types
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/Application/src/tracker/python"
tv = types.ModuleType("torchvision")
tv.__path__ = []
tvt = types.ModuleType("torchvision.transforms")
tvt.Normalize = lambda mean, std: None
tvm = types.ModuleType("torchvision.models")
tv.transforms, tv.models = tvt, tvm
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.models": tvm})
sys.path.insert(0, REF)
import visual_identification_network_torch as ref  # noqa: E402

from trex_amd import weights  # noqa: E402
from oracle import cnn_oracle  # noqa: E402
import identity_synth  # noqa: E402
import trained_net  # noqa: E402

DROPOUT_SEEDS = (101, 202, 303)


def run(ids, seed, epochs, val, test):
    torch.manual_seed(seed)
    model = ref.ModelFetcher().get_model("v118_3", ids.classes, 1, 80, 80, "cpu")
    sd = model.model.state_dict()
    for k, v in weights.synthetic_state(ids.classes, trained_net.WEIGHT_SEED).items():
        sd[k].copy_(torch.from_numpy(v))
    criterion = torch.nn.CrossEntropyLoss()
    optimizer = torch.optim.Adam(model.parameters(), lr=trained_net.LR)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.1, patience=5)
    vx, vy = torch.from_numpy(val[0].astype(np.float32)), torch.from_numpy(val[1]).long()
    hist = []
    for epoch in range(epochs):
        t0 = time.time()
        model.train()
        losses = []
        for x, y in ids.train_epoch(epoch):
            out = model(torch.from_numpy(x))
            loss = criterion(out.contiguous(), torch.from_numpy(y).long())
            loss.backward()
            optimizer.step()
            optimizer.zero_grad(set_to_none=True)
            losses.append(float(loss.detach()))
        model.eval()
        vl, vc = [], 0
        with torch.no_grad():
            for lo in range(0, len(vy), identity_synth.BATCH):
                out = model(vx[lo:lo + identity_synth.BATCH])
                vl.append(float(criterion(out, vy[lo:lo + identity_synth.BATCH])))
                vc += int((out.argmax(1) == vy[lo:lo + identity_synth.BATCH]).sum())
        val_loss = float(np.mean(vl))
        scheduler.step(val_loss)
        hist.append((float(np.mean(losses)), val_loss, vc / len(vy)))
        print(f"seed {seed} epoch {epoch}: loss {hist[-1][0]:.4f} val_loss {val_loss:.4f} val_acc {hist[-1][2]:.4f}  ({time.time() - t0:.0f} s)", flush=True)
    st = {k: v.numpy().copy() for k, v in model.model.state_dict().items() if "num_batches" not in k}
    probs, maxima = [], [[], [], []]
    for lo in range(0, len(test[1]), 256):
        p, _ = cnn_oracle.predict(st, test[0][lo:lo + 256], dtype=torch.float64)
        probs.append(p)
        for k, m in enumerate(cnn_oracle.stage_maxima(st, test[0][lo:lo + 256])):
            maxima[k].append(m)
    probs = np.concatenate(probs)
    acc, top = float((probs.argmax(1) == test[1]).mean()), float(probs.max(1).mean())
    quant = np.array([np.quantile(np.concatenate(m), [0.5, 0.99, 1.0]) for m in maxima])
    print(f"seed {seed}: test accuracy {acc:.4f}, mean top softmax {top:.4f}, stage maxima 50/99/100 %:\n{quant}", flush=True)
    return np.array(hist), acc, top, quant


def main():
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "8")))
    epochs = int(sys.argv[1]) if len(sys.argv) > 1 else trained_net.EPOCHS
    seeds = DROPOUT_SEEDS[:int(sys.argv[2])] if len(sys.argv) > 2 else DROPOUT_SEEDS
    ids = identity_synth.Identities(trained_net.CLASSES, trained_net.IDENTITY_SEED)
    val, test = ids.validation_set(), ids.test_set()
    runs = [run(ids, s, epochs, val, test) for s in seeds]
    for (h, acc, top, q), s in zip(runs, seeds):
        assert acc >= trained_net.MIN_ACCURACY and top >= trained_net.MIN_TOP_SOFTMAX, (s, acc, top)
        assert np.all(np.diff(h[:trained_net.MONO_EPOCHS, 0]) < 0), (s, h[:, 0])
    store = {"meta": np.array([trained_net.CLASSES, trained_net.IDENTITY_SEED, trained_net.WEIGHT_SEED, epochs, identity_synth.BATCHES_PER_EPOCH,
                               identity_synth.BATCH, trained_net.MONO_EPOCHS], np.int64),
             "dropout_seeds": np.array(seeds, np.int64),
             "history": np.stack([r[0] for r in runs]),                 # [seed][epoch][train loss, val loss, val accuracy]
             "test_accuracy": np.array([r[1] for r in runs]),
             "test_top_softmax": np.array([r[2] for r in runs]),
             "stage_quantiles": np.stack([r[3] for r in runs])}         # [seed][stage][50, 99, 100 %]
    fl, fa = store["history"][:, -1, 1], store["test_accuracy"]
    print(f"final validation loss {fl} (range width {np.ptp(fl):.4g}); test accuracy {fa} (range width {np.ptp(fa):.4g})")
    if len(seeds) == len(DROPOUT_SEEDS) and epochs == trained_net.EPOCHS:
        path = os.path.join(HERE, "cnn_trained_stats.npz")
        np.savez_compressed(path, **store)
        print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
