"""Side-car evaluator (resnet_cifar_main.py:361-421, resnet_cifar_eval.py,
resnet_imagenet_eval.py).

Polls `train_dir` for the newest checkpoint, restores it into an inference
model (GPU: the engine's forward-only plan with moving-average BN; CPU: the
fp32 model), scores `eval_batch_count` batches, logs

    precision: 0.933, best precision: 0.936
    precision@5: 0.997, best precision@5: 0.998

(the first line is the reference's, the second this project's top-5 line) and writes
`Precision` / `Best_Precision` and `Precision_top5` / `Best Precision_top5` scalar
summaries at the checkpoint's global_step into `eval_dir`.  The loss is the unsmoothed
cross-entropy whatever --label_smoothing the training run used.  `eval_once`
evaluates a single checkpoint and returns; otherwise it sleeps `eval_interval_secs`
(60 s in the reference) between polls and skips checkpoints it has already scored.
"""
from __future__ import annotations

import time

import torch

from ..ops.reference import in_top_k
from ..utils import tensor_bundle as tb
from ..utils.checkpoint import ema_weights, tf_to_state
from ..utils.records import EventWriter
from .hooks import log


class GPUInference:
    def __init__(self, spec, batch_size: int, device=None, ema: bool = False):
        from .engine import Engine, constant_lr

        self.ema = bool(ema)   # score the checkpoint's EMA shadows instead of its weights

        self.engine = Engine(spec, batch_size, weight_decay=0.0, lr_schedule=constant_lr(0.0),
                             device=device, use_graph=False)
        self.plan = self.engine.build_eval_plan(batch_size)
        # "persistent" (one prn_infer launch + softmax) or "per-layer" (tune persist_eval)
        self.eval_path = self.plan.kind
        self.last_top5 = 0.0   # in-top-5 count of the last run's valid rows

    def load(self, tensors):
        if self.ema:   # trainables := their shadows (KeyError if the checkpoint has none)
            tensors = ema_weights(tensors, self.engine.params)
        tf_to_state(tensors, self.engine.params, None, strict=True)
        self.engine.repack()

    def run(self, images, labels):
        raw = images.dtype == torch.uint8
        n, full = images.shape[0], self.engine.N
        if n < full:
            # a short last batch (an eval pipeline's remainder, e.g. several loader
            # workers over 390-image ImageNet validation shards): the static plan runs
            # the full batch with the first image repeated, and the loss / correct count
            # are taken from the valid rows' probabilities
            pad = full - n
            images = torch.cat([images, images[:1].expand(pad, *images.shape[1:])])
            labels_p = torch.cat([labels, labels[:1].expand(pad)])
            _, _, probs = self.plan.run(images.to(self.engine.device),
                                        labels_p.to(self.engine.device), raw_u8=raw)
            p = probs[:n].float()
            y = labels.to(p.device).long()
            loss = float(-torch.log(p.gather(1, y[:, None]).clamp_min(1e-30)).sum())
            correct = float((p.argmax(1) == y).sum())
            self.last_top5 = float(in_top_k(p, y, 5).sum())
            return loss, correct, probs[:n]
        loss, correct, probs = self.plan.run(images.to(self.engine.device),
                                             labels.to(self.engine.device), raw_u8=raw)
        self.last_top5 = self.plan.top5
        return loss, correct, probs

    # ---- device-resident eval split (CIFAR): no per-batch image copy
    def attach(self, images, labels):
        """Upload a whole eval split (uint8 [M,3,32,32] + labels) once; evaluate_checkpoint
        then scores it through run_resident."""
        self.plan.attach(images, labels)

    @property
    def attached(self) -> bool:
        return self.plan.resident_plan is not None

    def resident_batch_sizes(self):
        """Valid rows of every batch of the attached split (the last may be short)."""
        M, full = self.plan.records, self.engine.N
        return [min(full, M - i * full) for i in range(self.plan.resident_batches)]

    def run_resident(self, batch_index: int, n_valid: int):
        """run() on batch `batch_index` of the attached split, `n_valid` rows of it real
        (the plan pads a short last batch with the batch's first record)."""
        loss, correct, probs = self.plan.run_resident(batch_index)
        full = self.engine.N
        if n_valid < full:   # as run(): loss / correct from the valid rows' probabilities
            p = probs[:n_valid].float()
            y = self.plan.labels[:n_valid].long()
            loss = float(-torch.log(p.gather(1, y[:, None]).clamp_min(1e-30)).sum())
            correct = float((p.argmax(1) == y).sum())
            self.last_top5 = float(in_top_k(p, y, 5).sum())
            return loss, correct, probs[:n_valid]
        self.last_top5 = self.plan.top5
        return loss, correct, probs


class CPUInference:
    def __init__(self, spec, batch_size: int, ema: bool = False):
        from .backends import CPUBackend
        from .engine import constant_lr

        self.ema = bool(ema)

        self.backend = CPUBackend(spec, batch_size, weight_decay=0.0, lr_schedule=constant_lr(0.0))
        self.last_top5 = 0.0

    def load(self, tensors):
        if self.ema:
            tensors = ema_weights(tensors, self.backend.store)
        tf_to_state(tensors, self.backend.store, None, strict=True)

    def run(self, images, labels):
        loss, correct, probs = self.backend.evaluate_batch(images, labels)
        self.last_top5 = self.backend.last_eval_top5
        return loss, correct, probs


def make_inference(spec, batch_size: int, device: str = "auto", ema: bool = False):
    """``ema``: load() takes every trainable from its ``/ExponentialMovingAverage`` shadow
    (utils/checkpoint.py ema_weights); BN moving statistics stay the checkpoint's."""
    if device == "auto":
        device = "gpu" if torch.cuda.is_available() else "cpu"
    return (GPUInference(spec, batch_size, ema=ema) if device == "gpu"
            else CPUInference(spec, batch_size, ema=ema))


def evaluate_checkpoint(model, prefix: str, batches, eval_batch_count: int, top5: bool = False):
    """Restore `prefix`, score up to eval_batch_count batches -> (precision, loss, step),
    with ``top5`` -> (precision, loss, step, top-5 precision).
    A model with an attached device-resident split (GPUInference.attach) scores that
    split's batches, in order, instead of `batches()`."""
    tensors = tb.read_bundle(prefix)
    model.load(tensors)
    step = int(tensors.get("global_step", 0))
    total = correct = loss = in5 = 0.0
    if getattr(model, "attached", False):   # the split already lives on the device
        for i, n in enumerate(model.resident_batch_sizes()[:eval_batch_count]):
            l, c, _ = model.run_resident(i, n)
            loss += l
            correct += c
            in5 += model.last_top5
            total += n
    else:
        for i, (x, y) in enumerate(batches()):
            if i >= eval_batch_count:
                break
            l, c, _ = model.run(x, y)
            loss += l
            correct += c
            in5 += getattr(model, "last_top5", 0.0)
            total += y.shape[0]
    out = (correct / max(total, 1.0)), (loss / max(total, 1.0)), step
    return out + (in5 / max(total, 1.0),) if top5 else out


class SidecarEvaluator:
    def __init__(self, model, batches, train_dir: str, eval_dir: str | None,
                 eval_batch_count: int = 50, eval_once: bool = False,
                 interval_s: float = 60.0, exit_if_no_checkpoint: bool = False):
        self.model = model
        self.batches = batches
        self.train_dir = train_dir
        self.writer = EventWriter(eval_dir) if eval_dir else None
        self.count = eval_batch_count
        self.once = eval_once
        self.interval = interval_s
        self.exit_if_none = exit_if_no_checkpoint
        self.best = 0.0
        self.best_top5 = 0.0
        self.last_prefix = None
        self.history = []        # (step, precision, loss) per scored checkpoint
        self.history_top5 = []   # its top-5 precision
        if getattr(model, "ema", False):
            log("INFO:tensorflow:weights: ema")
        path = getattr(model, "eval_path", None)
        if path is not None:
            log(f"INFO:tensorflow:eval forward path: {path}")

    def run(self, max_polls: int | None = None):
        polls = 0
        while True:
            polls += 1
            prefix = tb.latest_checkpoint(self.train_dir)
            if prefix is None:
                log(f"INFO:tensorflow:No model to eval yet at {self.train_dir}")
                if self.exit_if_none or self.once:
                    return self.history
            elif prefix != self.last_prefix:
                prec, loss, step, prec5 = evaluate_checkpoint(self.model, prefix, self.batches,
                                                              self.count, top5=True)
                self.best = max(self.best, prec)
                self.best_top5 = max(self.best_top5, prec5)
                self.last_prefix = prefix
                self.history.append((step, prec, loss))
                self.history_top5.append(prec5)
                log(f"INFO:tensorflow:loss: {loss:.3f}, precision: {prec:.3f}, "
                    f"best precision: {self.best:.3f}")
                log(f"INFO:tensorflow:precision@5: {prec5:.3f}, "
                    f"best precision@5: {self.best_top5:.3f}")
                if self.writer is not None:
                    self.writer.add_scalars(step, {"Precision": prec, "Best_Precision": self.best,
                                                   "Precision_top5": prec5,
                                                   "Best Precision_top5": self.best_top5})
                    self.writer.flush()
                if self.once:
                    return self.history
            if max_polls is not None and polls >= max_polls:
                return self.history
            time.sleep(self.interval)
