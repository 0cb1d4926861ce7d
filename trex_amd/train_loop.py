"""Host side of the identity network's training, with the interface of the reference's Python (the reference's host side of this path is
Python too): the epoch loop of train() (Application/src/tracker/python/visual_recognition_torch.py:1036-1283) on top of
capi.Trainer -- whose step / evaluate replace the loop's body (:1137-1158 and :1171-1190) -- and the learning-rate schedule it is handed
(optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor=0.1, patience=5), :1425).

What stays with the caller, as in the reference: the loaders (any iterable of (inputs NHWC float32 in [0, 255], integer targets) with a
len(), e.g. the reference's own DataLoader over TRexImageDataset with its augmentation, :158-188, :1325-1411) and the callback object
(ValidationCallback, :355-560: per-class accuracy, uniqueness, early stopping), used through the same three members train() uses:
on_batch_end(batch, logs), on_epoch_end(epoch, logs), stop_training.  No torch in here: batches may be numpy arrays or anything
np.asarray() accepts (torch CPU tensors included).

Or the loader runs on the device: ResidentLoader keeps the uint8 crops in HBM and makes every batch there (trexhip_augment_device: the
reference's RandomAffine + ColorJitter, or the plain conversion of the validation loader), and train_resident() is the same epoch loop
over the device pointers it yields, so an epoch never leaves the device.

The measurements of the callback can stay there too: ResidentValidation keeps the validation crops and the crops of the uniqueness
estimate in HBM, predicts them with the weights as they stand in the trainer (trexhip_train_predict_device) and reduces the rows on the
device (trexhip_validation_metrics_device) to what ValidationCallback.evaluate records per epoch (:510-543): the accuracy of each class
and estimate_uniqueness().  The stop rules (:545-650) read TRex globals that this library does not own: they stay with the caller.

ResidentAverages does the same for the question accumulation asks per candidate range (Accumulation::check_additional_range ->
VINetwork::paverages, ml/VisualIdentification.h:145-180): the mean probability row of every individual over its crops, predicted and
averaged in HBM (trexhip_class_averages_device).  The decision made from it is C++ in the reference and here (host/HipAccumulation.h).
"""
import numpy as np


class ReduceLROnPlateau:
    """torch.optim.lr_scheduler.ReduceLROnPlateau for one learning rate (pinned against torch's in tests/test_train_loop.py).
    step(metric) -> the learning rate to use from now on."""

    def __init__(self, lr, mode="min", factor=0.1, patience=5, threshold=1e-4, threshold_mode="rel", cooldown=0, min_lr=0.0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if mode not in ("min", "max") or threshold_mode not in ("rel", "abs"):
            raise ValueError("mode / threshold_mode")
        self.lr, self.mode, self.factor, self.patience = float(lr), mode, factor, patience
        self.threshold, self.threshold_mode, self.cooldown, self.min_lr, self.eps = threshold, threshold_mode, cooldown, min_lr, eps
        self.best = float("inf") if mode == "min" else -float("inf")
        self.num_bad_epochs = 0
        self.cooldown_counter = 0
        self.last_epoch = 0

    def _is_better(self, a, best):
        if self.mode == "min" and self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold)
        if self.mode == "min":
            return a < best - self.threshold
        if self.threshold_mode == "rel":
            return a > best * (self.threshold + 1.0)
        return a > best + self.threshold

    def step(self, metric):
        current = float(metric)
        self.last_epoch += 1
        if self._is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            new_lr = max(self.lr * self.factor, self.min_lr)
            if self.lr - new_lr > self.eps:
                self.lr = new_lr
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        return self.lr

    def get_last_lr(self):
        return [self.lr]


def _host_batch(inputs, targets, check_shape):
    x = np.ascontiguousarray(np.asarray(inputs), np.float32)
    y = np.asarray(targets)
    if check_shape and (x.ndim != 4 or y.ndim != 1 or x.shape[0] != y.shape[0]):
        raise ValueError(f"Expected inputs (N,H,W,C) and targets (N,), got {x.shape} and {y.shape}")          # train() asserts the same, :1104-1112
    if y.dtype.kind not in "iu":
        raise ValueError(f"targets must be integer class indices, got {y.dtype}")     # train() asserts integer labels, :1109-1110
    return x, y.astype(np.int32), x.shape[0]


def _epochs(trainer, train_loader, val_loader, callback, scheduler, settings, abort, log, step, evaluate):
    """The epoch loop both entry points share.  step(batch) / evaluate(batch) -> (loss, correct, n) for whatever the loaders yield."""
    history = []
    best_val_acc = 0.0
    for epoch in range(int(settings["epochs"])):
        running_loss = 0.0
        running_acc = 0.0
        n_batches = 0
        for batch, item in enumerate(train_loader):
            loss, correct, n = step(item)
            acc = correct / float(n)
            running_loss += loss
            running_acc += acc
            n_batches += 1
            callback.on_batch_end(batch, {"loss": loss, "acc": acc})
        running_loss /= max(n_batches, 1)
        acc = running_acc / max(n_batches, 1)
        if len(val_loader) > 0:
            val_loss, correct, total, nb = 0.0, 0, 0, 0
            for item in val_loader:
                l, c, n = evaluate(item)
                val_loss += l
                correct += c
                total += n
                nb += 1
            val_loss /= nb
            val_acc = correct / float(total)
            best_val_acc = max(best_val_acc, val_acc)
            lr = scheduler.step(val_loss) if scheduler is not None else None
            if lr is not None:
                trainer.set_lr(lr)
            logs = {"val_loss": val_loss, "val_acc": val_acc, "val_precision": 0, "val_recall": 0}
            callback.on_epoch_end(epoch, logs)
            history.append({"epoch": epoch, "loss": running_loss, "acc": acc, **logs, "lr": lr})
        else:
            logs = {"loss": running_loss, "acc": acc}
            callback.on_epoch_end(epoch, logs)
            history.append({"epoch": epoch, **logs})
        if log is not None:
            log(f"Epoch {epoch}/{settings['epochs']} - " + " - ".join(f"{k}: {v}" for k, v in history[-1].items() if k != "epoch"))
        if getattr(callback, "stop_training", False):
            break
        if abort():
            break
    return history


def train(trainer, train_loader, val_loader, callback, scheduler, settings, abort=lambda: False, log=None):
    """The loop of train(model, train_loader, val_loader, criterion, optimizer, callback, scheduler, settings, device) with model +
    criterion + optimizer = `trainer` (capi.Trainer).  settings["epochs"] epochs; per batch one optimizer step and
    callback.on_batch_end(batch, {'loss', 'acc'}); per epoch the validation pass in eval mode (when val_loader is not empty), scheduler.step(val_loss)
    -> trainer.set_lr, callback.on_epoch_end(epoch, logs); stops when callback.stop_training or abort() is set.  Returns the history."""
    def step(item):
        x, y, n = _host_batch(item[0], item[1], True)
        return (*trainer.step(x, y), n)

    def evaluate(item):
        x, y, n = _host_batch(item[0], item[1], False)
        return (*trainer.evaluate(x, y), n)

    return _epochs(trainer, train_loader, val_loader, callback, scheduler, settings, abort, log, step, evaluate)


def train_resident(trainer, train_loader, val_loader, callback, scheduler, settings, abort=lambda: False, log=None):
    """train() over loaders that yield device memory -- (d_inputs_ptr, d_targets_ptr, n), e.g. ResidentLoader --: one
    Trainer.step_device per batch, Trainer.evaluate_device per validation batch; everything else as in train()."""
    def step(item):
        return (*trainer.step_device(item[0], item[1], item[2]), item[2])

    def evaluate(item):
        return (*trainer.evaluate_device(item[0], item[1], item[2]), item[2])

    return _epochs(trainer, train_loader, val_loader, callback, scheduler, settings, abort, log, step, evaluate)


class ResidentLoader:
    """TRexImageDataset + DataLoader (visual_recognition_torch.py:158-194, :1391-1410) with the samples in HBM.

    crops_uint8: uint8 array (N, H, W, C), uploaded once -- or a device address of such a pool, e.g. what the crop calls wrote, with
    count=N and image_shape=(H, W, C).  targets: integer array (N,), or a device address of N int32 when crops_uint8 is one.
    Iterating yields (d_inputs_ptr, d_targets_ptr, n) per batch: float32 [n][H][W][C] in [0, 255] and int32 [n], made by ONE
    trexhip_augment_device call each, in the loader's own two buffers (the next batch overwrites them; calls on the context are
    ordered, so a step that was handed a batch has read it before the next is written).  Every epoch draws a new seeded permutation
    when shuffle is set and new augmentations (the call's counter runs on); drop_last=False: the last batch may be smaller.
    augment=True applies `params` (default: capi.default_augment_params(W, H), the reference's transform); augment=False,
    shuffle=False is the validation loader.  `rows` (pool indices, default: all of them) restricts what is served to a subset of the pool -- the
    training or the validation rows of one resident pool.  `seg` is the capi.Segmenter whose stream the trainer uses."""

    def __init__(self, seg, crops_uint8, targets, batch_size, augment=True, shuffle=True, seed=0, count=None, image_shape=None, params=None, rows=None):
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.seg, self.batch_size, self.shuffle, self.seed = seg, int(batch_size), bool(shuffle), int(seed)
        self._owned = []
        if isinstance(crops_uint8, (int, np.integer)):
            if count is None or image_shape is None or not isinstance(targets, (int, np.integer)):
                raise ValueError("a device pool needs count, image_shape=(H, W, C) and a device address of its int32 targets")
            self.count, (self.height, self.width, self.channels) = int(count), (int(v) for v in image_shape)
            self.d_pool, self.d_pool_targets = int(crops_uint8), int(targets)
        else:
            x = np.asarray(crops_uint8)
            y = np.asarray(targets)
            if x.dtype != np.uint8 or x.ndim != 4:
                raise ValueError(f"crops must be uint8 (N, H, W, C), got {x.dtype} {x.shape}")
            if y.dtype.kind not in "iu" or y.shape != (x.shape[0],):
                raise ValueError(f"targets must be integer class indices of shape ({x.shape[0]},), got {y.dtype} {y.shape}")
            self.count, self.height, self.width, self.channels = (int(v) for v in x.shape)
            self.d_pool = self._alloc(max(x.nbytes, 1))
            self.d_pool_targets = self._alloc(4 * max(self.count, 1))
            if self.count:
                seg.copy_to_device(self.d_pool, x)
                seg.copy_to_device(self.d_pool_targets, y.astype(np.int32))
        self.rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
        if self.rows is not None and self.rows.size and (self.rows.min() < 0 or self.rows.max() >= self.count):
            raise ValueError("rows must be indices into the pool")
        self.params = None
        if augment:
            if params is None:
                from . import capi
                params = capi.default_augment_params(self.width, self.height)
            params.seed = self.seed
            self.params = params
        self.d_inputs = self._alloc(4 * self.batch_size * self.height * self.width * self.channels)
        self.d_targets = self._alloc(4 * self.batch_size)
        self.epoch = 0
        self.calls = 0

    def _alloc(self, nbytes):
        p = self.seg.device_alloc(nbytes)
        self._owned.append(p)
        return p

    def __len__(self):
        served = self.count if self.rows is None else len(self.rows)
        return (served + self.batch_size - 1) // self.batch_size

    def order(self, epoch):
        """pool indices of `epoch` in the order they are served"""
        rows = np.arange(self.count, dtype=np.int32) if self.rows is None else self.rows
        if not self.shuffle:
            return rows
        return rows[np.random.default_rng([self.seed, epoch]).permutation(len(rows))].astype(np.int32)

    def __iter__(self):
        order = self.order(self.epoch)
        self.epoch += 1
        for b in range(len(self)):
            idx = order[b * self.batch_size:(b + 1) * self.batch_size]
            self.seg.augment_device(self.d_pool, self.count, len(idx), self.width, self.height, self.channels, self.d_inputs, ap=self.params, indices=idx,
                                    d_pool_targets_ptr=self.d_pool_targets, d_targets_out_ptr=self.d_targets, counter=self.calls)
            self.calls += 1
            yield self.d_inputs, self.d_targets, len(idx)

    def close(self):
        for p in self._owned:
            self.seg.device_free(p)
        self._owned = []


def train_category(seg, weight_blob, crops_uint8, targets, validation_indexes, epochs=10, batch_size=32, lr=1e-4, seed=0, keep_masks=None, history=None,
                   log=None):
    """Categorize.perform_training (trex_learn_category.py:276-340) without leaving the device: the labelled crops (uint8 (N, H, W, C), targets (N,))
    are uploaded once as a resident pool; the training rows are the pool without `validation_indexes` (:291-294); `epochs` epochs (10) of batches of
    `batch_size` (32) over a shuffled index list per epoch (DataLoader(shuffle=True), :312 -- here ResidentLoader's seeded permutation, augment=False:
    the reference feeds the crops as they are), one Adam step at `lr` (1e-4, :295) per batch and the epoch's mean of the batch losses (:334-336); then the
    evaluation of update_best_accuracy (:356-391) on the validation rows in eval mode: the mean loss over the samples and the accuracy.  Returns the
    exported 'TRXC' blob, which trexhip_categorize_load_weights takes.

    weight_blob: the network to start from (a fresh one: weights.pack_category_blob of an initialisation).  keep_masks(epoch, batch, n) -> packed uint8
    masks of that step or None (the library draws them): how a test injects what a restatement used.  history, when a dict, receives "losses" (per
    epoch), "val_loss", "val_accuracy" and "steps".  What stays with the caller, as it is GUI and file business in the reference: choosing the
    validation split (:232-260), the "500 new samples" rule that decides WHEN to train, the checkpoint file with the sample store (:342-351), and
    classification_report beyond the accuracy."""
    from . import capi
    x = np.asarray(crops_uint8)
    y = np.asarray(targets)
    val = np.unique(np.asarray(validation_indexes, np.int64))
    train_rows = np.delete(np.arange(len(x), dtype=np.int64), val)
    if not len(train_rows):
        raise ValueError("no training rows are left beside the validation rows")
    trainer = capi.Trainer(seg, weight_blob, max_batch=batch_size, lr=lr, seed=seed)
    if trainer.version != capi.Trainer.NET_CATEGORY:
        trainer.close()
        raise ValueError("train_category needs a category blob ('TRXC')")
    train = ResidentLoader(seg, x, y, batch_size, augment=False, shuffle=True, seed=seed, rows=train_rows)
    # the validation rows out of the same resident pool
    valid = ResidentLoader(seg, train.d_pool, train.d_pool_targets, batch_size, augment=False, shuffle=False, count=train.count,
                           image_shape=(train.height, train.width, train.channels), rows=val)
    d_keep = seg.device_alloc(max(trainer.keep_mask_bytes(batch_size), 1)) if keep_masks is not None else 0
    try:
        losses = []
        for epoch in range(epochs):
            running = 0.0
            for b, (d_x, d_y, n) in enumerate(train):
                k = keep_masks(epoch, b, n) if keep_masks is not None else None
                if k is not None:
                    k = np.ascontiguousarray(k, np.uint8)
                    if k.size != trainer.keep_mask_bytes(n):
                        raise ValueError(f"keep_masks({epoch}, {b}, {n}) holds {k.size} bytes, the step needs {trainer.keep_mask_bytes(n)}")
                    seg.copy_to_device(d_keep, k)
                running += trainer.step_device(d_x, d_y, n, d_keep if k is not None else 0)[0]
            losses.append(running / len(train))
            if log:
                log(f"Epoch {epoch + 1}, Loss: {losses[-1]}")
        total_loss, total_correct, count = 0.0, 0, 0
        for d_x, d_y, n in valid:
            loss, correct = trainer.evaluate_device(d_x, d_y, n)
            total_loss += loss * n
            total_correct += correct
            count += n
        if history is not None:
            history.update(losses=losses, val_loss=total_loss / max(count, 1), val_accuracy=total_correct / max(count, 1), steps=trainer.steps)
        return trainer.export()
    finally:
        if d_keep:
            seg.device_free(d_keep)
        valid.close()
        train.close()
        trainer.close()


class _PerClassHistory(dict):
    """ValidationCallback.per_class_accuracy, {class: [accuracy of every epoch]} (:522-525); calling it measures the accuracies now."""

    def __init__(self, measure):
        super().__init__()
        self._measure = measure

    def __call__(self):
        return self._measure()


class ResidentValidation:
    """What ValidationCallback.evaluate measures at the end of an epoch (visual_recognition_torch.py:493-543), with the samples in HBM and
    the weights where they are, in the trainer: no export, no second copy of the network, one device-to-host copy of the results.

    val_crops_uint8 (N, H, W, C) uint8 at the trainer's individual_image_size (trainer.height, trainer.width) + val_targets (N,): the validation
    images (X_test / Y_test); unique_crops_uint8 (M, H, W, C) +
    frame_ranges (F, 2) = (start, end) rows of it per frame, in frame order: what Accumulation hands calculate_uniqueness (_disc_images,
    _disc_frame_map, ui/Accumulation.cpp:900-901).  Arrays are uploaded once; like ResidentLoader, device addresses are taken as they
    are with count= (validation pool, targets then a device address of int32) and unique_count=.  Either part may be missing.
      per_class_accuracy()      -> float64 [classes], plot_comparison_raw's column 3 (:406-451)
      estimate_uniqueness()     -> float, the third element of calculate_uniqueness's tuple, as step_calculate_uniqueness returns it
      on_epoch_end(epoch, logs) appends to per_class_accuracy[i], mean_values, worst_values and uniquenesses as :522-543 does, then
                                forwards to `callback` (the caller's ValidationCallback with its stop rules), if there is one
      on_batch_end, stop_training  delegate to `callback`
    so it can be train_resident()'s callback itself, or its two measurements can be plugged into the caller's own."""

    def __init__(self, trainer, seg, val_crops_uint8, val_targets, unique_crops_uint8=None, frame_ranges=None, count=None, unique_count=None, callback=None):
        self.trainer, self.seg, self.callback = trainer, seg, callback
        self.classes, self.channels = trainer.classes, trainer.channels
        self.height, self.width = trainer.height, trainer.width
        self._owned = []
        self.d_val, self.n_val = self._pool(val_crops_uint8, count)
        self.d_val_targets = 0
        if self.n_val:
            if isinstance(val_targets, (int, np.integer)):
                self.d_val_targets = int(val_targets)
            else:
                y = np.asarray(val_targets)
                if y.dtype.kind not in "iu" or y.shape != (self.n_val,):
                    raise ValueError(f"val_targets must be integer class indices of shape ({self.n_val},), got {y.dtype} {y.shape}")
                self.d_val_targets = self._alloc(4 * self.n_val)
                seg.copy_to_device(self.d_val_targets, y.astype(np.int32))
        self.d_unique, self.n_unique = self._pool(unique_crops_uint8, unique_count)
        self.frame_ranges = None
        if self.n_unique:
            if frame_ranges is None:
                raise ValueError("the crops of the uniqueness estimate need frame_ranges")
            self.frame_ranges = np.ascontiguousarray(frame_ranges, np.int32).reshape(-1, 2)
        self.d_probs = self._alloc(4 * self.classes * max(self.n_val, self.n_unique, 1))
        self.per_class_accuracy = _PerClassHistory(self._measure_per_class_accuracy)
        self.mean_values, self.worst_values, self.uniquenesses = [], [], []
        self.last_validation = self.last_uniqueness = None          # the ValidationMetrics of the last measurement of each kind
        self._stop = False

    def _alloc(self, nbytes):
        p = self.seg.device_alloc(nbytes)
        self._owned.append(p)
        return p

    def _pool(self, crops, count):
        if crops is None:
            return 0, 0
        if isinstance(crops, (int, np.integer)):
            if count is None:
                raise ValueError("a device pool needs its count")
            return int(crops), int(count)
        x = np.asarray(crops)
        if x.dtype != np.uint8 or x.ndim != 4 or tuple(x.shape[1:]) != (self.height, self.width, self.channels):
            raise ValueError(f"crops must be uint8 (N, {self.height}, {self.width}, {self.channels}), got {x.dtype} {x.shape}")
        if x.shape[0] == 0:
            return 0, 0
        d = self._alloc(x.nbytes)
        self.seg.copy_to_device(d, x)
        return d, int(x.shape[0])

    def _measure_per_class_accuracy(self):
        if not self.n_val:
            raise ValueError("no validation crops")
        self.trainer.predict_device(self.d_val, self.n_val, self.d_probs)
        self.last_validation = self.seg.validation_metrics(self.d_probs, self.n_val, self.classes, d_targets_ptr=self.d_val_targets)
        return self.last_validation.per_class_accuracy

    def estimate_uniqueness(self):
        if not self.n_unique:
            raise ValueError("no crops for the uniqueness estimate")
        self.trainer.predict_device(self.d_unique, self.n_unique, self.d_probs)
        self.last_uniqueness = self.seg.validation_metrics(self.d_probs, self.n_unique, self.classes, frame_ranges=self.frame_ranges)
        return self.last_uniqueness.mean_unique

    def on_batch_end(self, batch, logs):
        if self.callback is not None:
            self.callback.on_batch_end(batch, logs)

    def on_epoch_end(self, epoch, logs):
        if self.n_val:
            acc = self.per_class_accuracy()
            for i in range(len(acc)):
                self.per_class_accuracy.setdefault(i, []).append(acc[i])
            self.mean_values.append(np.mean(acc))
            self.worst_values.append(np.min(acc))
        if self.n_unique:
            self.uniquenesses.append(self.estimate_uniqueness())
        if self.callback is not None:
            self.callback.on_epoch_end(epoch, logs)

    @property
    def stop_training(self):
        return self._stop or bool(getattr(self.callback, "stop_training", False))

    @stop_training.setter
    def stop_training(self, value):
        self._stop = bool(value)

    def close(self):
        for p in self._owned:
            self.seg.device_free(p)
        self._owned = []


class ResidentAverages:
    """VINetwork::paverages (ml/VisualIdentification.h:145-180) with the crops of a candidate range and their ids in HBM: one prediction, one
    reduction on the device, one device-to-host copy of individuals x classes floats.

    predict(d_crops, n, d_probs): trainer.predict_device (the weights as they stand in the trainer) or seg.identify_device (the loaded
    network); classes: the width of its rows (None: the trainer's, or the loaded network's).  crops_uint8 (N, H, W, C) uint8 + ids (N,) integers, any values: they are mapped to dense keys
    in ascending order, as the reference's std::map orders them, and uploaded once.  Like ResidentValidation, device addresses are taken as
    they are with count=: crops_uint8 a device address, ids a device address of int32 dense keys 0..n_ids-1, id_values the n_ids ids the
    keys stand for.
      averages() -> {id: (samples float32, values float32 [classes])} in id order; an id without rows is absent, as in the reference.
                    Bit for bit what the host loop gives on the same rows.  The ClassAverages of the call (with max_index / max_p of
                    check_additional_range's scan, by dense key) stays in last."""

    def __init__(self, predict, seg, crops_uint8, ids, classes=None, count=None, id_values=None):
        if classes is None:                                  # the trainer knows its classes, the segmenter those of the loaded network
            owner = getattr(predict, "__self__", None)
            classes = owner.classes if hasattr(owner, "classes") else seg.num_classes()
        self.predict, self.seg, self.classes = predict, seg, int(classes)
        self._owned = []
        self.last = None
        if isinstance(crops_uint8, (int, np.integer)):
            if count is None or id_values is None or not isinstance(ids, (int, np.integer)):
                raise ValueError("a device pool needs its count, a device address of dense int32 keys and id_values")
            self.d_crops, self.n, self.d_keys = int(crops_uint8), int(count), int(ids)
            self.id_values = [int(v) for v in id_values]
        else:
            x = np.asarray(crops_uint8)
            y = np.asarray(ids)
            if x.dtype != np.uint8 or x.ndim != 4:
                raise ValueError(f"crops must be uint8 (N, H, W, C), got {x.dtype} {x.shape}")
            owner = getattr(predict, "__self__", None)           # a trainer's predict_device reads crops of the trainer's own size
            if hasattr(owner, "height") and tuple(x.shape[1:]) != (owner.height, owner.width, owner.channels):
                raise ValueError(f"crops must be uint8 (N, {owner.height}, {owner.width}, {owner.channels}) for this trainer, got {x.shape}")
            if y.dtype.kind not in "iu" or y.shape != (x.shape[0],):
                raise ValueError(f"ids must be integers of shape ({x.shape[0]},), got {y.dtype} {y.shape}")
            values, keys = np.unique(y, return_inverse=True)
            self.id_values = [int(v) for v in values]
            self.n = int(x.shape[0])
            self.d_crops = self.d_keys = 0
            if self.n:
                self.d_crops = self._alloc(x.nbytes)
                seg.copy_to_device(self.d_crops, x)
                self.d_keys = self._alloc(4 * self.n)
                seg.copy_to_device(self.d_keys, keys.astype(np.int32))
        self.d_probs = self._alloc(4 * self.classes * max(self.n, 1))

    def _alloc(self, nbytes):
        p = self.seg.device_alloc(nbytes)
        self._owned.append(p)
        return p

    def averages(self):
        if not self.n:
            return {}
        self.predict(self.d_crops, self.n, self.d_probs)
        self.last = self.seg.class_averages(self.d_probs, self.n, self.classes, self.d_keys, len(self.id_values))
        return {v: (self.last.samples[k], self.last.values[k]) for k, v in enumerate(self.id_values) if self.last.samples[k] > 0}

    def close(self):
        for p in self._owned:
            self.seg.device_free(p)
        self._owned = []
