"""tf.train.Saver / CheckpointSaverHook equivalent over the tensor-bundle codec.

Variables saved exactly as the reference's MonitoredTrainingSession did
(403 entries for CIFAR ResNet-50): every trainable
under its TF name (HWIO conv kernels, BN gamma/beta, dense kernel/bias), its
``<name>/Momentum`` optimizer slot, the BN moving statistics and the int64
``global_step``; a run with ``--ema_decay`` adds ``<name>/ExponentialMovingAverage`` per
trainable (tf.train.ExponentialMovingAverage's shadow variables); a run with ``--optimizer
adamw`` saves ``<name>/Adam`` and ``<name>/Adam_1`` in place of ``<name>/Momentum``, plus
``beta1_power``, ``beta2_power`` and ``adam_start_step``; a run with ``--optimizer lion``
saves ``<name>/Lion`` in place of ``<name>/Momentum`` (no extra scalars); a run with
``--optimizer rmsprop`` saves tf.train.RMSPropOptimizer's slots in their creation order
(``rms``, then ``mg`` if centered, then ``momentum``): ``<name>/RMSProp`` and
``<name>/RMSProp_1``, centered ``<name>/RMSProp``, ``<name>/RMSProp_1`` and
``<name>/RMSProp_2``, in place of ``<name>/Momentum`` (no extra scalars).  ``max_to_keep``
= 5, the ``checkpoint`` state file lists the retained prefixes, files are written to temporaries and renamed (a killed
writer never leaves a half checkpoint that restore would pick up).
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import tensor_bundle as tb


EMA_SUFFIX = "/ExponentialMovingAverage"   # tf.train.ExponentialMovingAverage's shadow name


ADAM_M_SUFFIX, ADAM_V_SUFFIX = "/Adam", "/Adam_1"   # tf.train.AdamOptimizer's slot names
ADAM_START = "adam_start_step"                     # ours: the step the moments count from


LION_SUFFIX = "/Lion"   # lion's one slot: an average of the gradient, not mom's accumulator


# tf.train.RMSPropOptimizer's slot names, in the order TF 1.12 creates the slots: rms, mg
# (centered only), momentum -- so "/RMSProp_1" is the momentum of a plain run and mg of a
# centered one
RMSPROP_SUFFIXES = ("/RMSProp", "/RMSProp_1", "/RMSProp_2")


def rmsprop_suffixes(centered: bool) -> dict:
    """{"ms", "mom"[, "mg"]: slot suffix} of a plain or centered rmsprop run."""
    if centered:
        return {"ms": RMSPROP_SUFFIXES[0], "mg": RMSPROP_SUFFIXES[1], "mom": RMSPROP_SUFFIXES[2]}
    return {"ms": RMSPROP_SUFFIXES[0], "mom": RMSPROP_SUFFIXES[1]}


def adam_beta_powers(t_done: int, beta1: float, beta2: float):
    """TF 1.12's beta1_power / beta2_power variables after t_done Adam steps: b^(t_done + 1)
    (they start at b and are multiplied by b after every step), from the fp32 betas in fp64,
    as fp32."""
    return (np.float32(float(np.float32(beta1)) ** (int(t_done) + 1)),
            np.float32(float(np.float32(beta2)) ** (int(t_done) + 1)))


def state_to_tf(store, momentum: torch.Tensor | None, global_step: int,
                ema: torch.Tensor | None = None, adam: dict | None = None,
                lion: bool = False, rmsprop: dict | None = None) -> dict[str, np.ndarray]:
    """ParamStore (+flat momentum, +flat EMA shadows, in the same layout) -> {TF name: array}.
    ``ema`` adds ``<name>/ExponentialMovingAverage`` per trainable; without it the entries
    are exactly the reference's.  ``adam`` (an adamw run: {"v": flat second moment,
    "start_step", "beta1", "beta2"}): `momentum` is the first moment and goes out as
    ``<name>/Adam``, v as ``<name>/Adam_1`` (TF's slot names), no ``/Momentum``; plus the fp32
    scalars beta1_power / beta2_power (TF 1.12's variables after global_step - start_step
    Adam steps) and the int64 ``adam_start_step``, which restore goes by.  ``lion`` (a lion
    run): `momentum` is its m and goes out as ``<name>/Lion``, no ``/Momentum``.  ``rmsprop``
    (an rmsprop run: {"ms": flat mean square, "mg": flat mean gradient or None}): `momentum`,
    ms and mg go out under rmsprop_suffixes(mg is not None), no ``/Momentum``."""
    out: dict[str, np.ndarray] = {}
    master = store.master.detach().float().cpu().numpy()
    stats = store.stats.detach().float().cpu().numpy()
    mom = momentum.detach().float().cpu().numpy() if momentum is not None else None
    sh = ema.detach().float().cpu().numpy() if ema is not None else None
    v = adam["v"].detach().float().cpu().numpy() if adam is not None else None
    m_suffix = ADAM_M_SUFFIX if adam is not None else LION_SUFFIX if lion else "/Momentum"
    rms = {}
    if rmsprop is not None:
        suf = rmsprop_suffixes(rmsprop.get("mg") is not None)
        m_suffix = suf["mom"]
        rms = {suf[k]: rmsprop[k].detach().float().cpu().numpy() for k in suf if k != "mom"}
    for s in store.train_slots:
        out[s.name] = master[s.offset:s.offset + s.numel].reshape(s.shape).copy()
        if mom is not None:
            out[s.name + m_suffix] = mom[s.offset:s.offset + s.numel].reshape(s.shape).copy()
        for suffix, buf in rms.items():
            out[s.name + suffix] = buf[s.offset:s.offset + s.numel].reshape(s.shape).copy()
        if v is not None:
            out[s.name + ADAM_V_SUFFIX] = v[s.offset:s.offset + s.numel].reshape(s.shape).copy()
        if sh is not None:
            out[s.name + EMA_SUFFIX] = sh[s.offset:s.offset + s.numel].reshape(s.shape).copy()
    for s in store.stat_slots:
        out[s.name] = stats[s.offset:s.offset + s.numel].reshape(s.shape).copy()
    out["global_step"] = np.array(int(global_step), dtype=np.int64)
    if adam is not None:
        start = int(adam["start_step"])
        p1, p2 = adam_beta_powers(int(global_step) - start, adam["beta1"], adam["beta2"])
        out["beta1_power"], out["beta2_power"] = np.array(p1), np.array(p2)
        out[ADAM_START] = np.array(start, dtype=np.int64)
    return out


def tf_to_adam(tensors: dict, store, m: torch.Tensor, v: torch.Tensor) -> int:
    """Load the two Adam moments of an adamw run from {TF name: array}; returns the step the
    bias correction counts from.  With every ``<name>/Adam`` and ``<name>/Adam_1`` present:
    both are loaded and the start step is the checkpoint's ``adam_start_step`` (0 without
    that entry: a file TF wrote).  Otherwise (e.g. a `mom` checkpoint, whose ``/Momentum`` is
    ignored): both moments are zero and the start step is the checkpoint's global_step, so
    the bias correction restarts with the moments; one log line says so."""
    gs = int(np.asarray(tensors.get("global_step", 0)))
    absent = [s.name for s in store.train_slots
              if s.name + ADAM_M_SUFFIX not in tensors or s.name + ADAM_V_SUFFIX not in tensors]
    if absent:
        print(f"INFO:tensorflow:checkpoint has no Adam slots for {len(absent)} of "
              f"{len(store.train_slots)} variables (e.g. {absent[0] + ADAM_M_SUFFIX}): both moments "
              f"start from zero and the bias correction restarts at step {gs}", flush=True)
        m.data.zero_()
        v.data.zero_()
        return gs
    for buf, suffix in ((m, ADAM_M_SUFFIX), (v, ADAM_V_SUFFIX)):
        for s in store.train_slots:
            a = np.asarray(tensors[s.name + suffix], dtype=np.float32).reshape(-1)
            if a.size != s.numel:
                raise ValueError(f"{s.name + suffix}: {a.size} elements, expected {s.numel}")
            buf.data[s.offset:s.offset + s.numel].copy_(torch.from_numpy(a))
    return int(np.asarray(tensors.get(ADAM_START, 0)))


def tf_to_lion(tensors: dict, store, m: torch.Tensor) -> None:
    """Load the m of a lion run from {TF name: array}.  With every ``<name>/Lion`` present it
    is loaded; otherwise (e.g. a `mom` checkpoint, whose ``/Momentum`` is an accumulator and
    is ignored) m is zero and one log line says so."""
    absent = [s.name for s in store.train_slots if s.name + LION_SUFFIX not in tensors]
    if absent:
        print(f"INFO:tensorflow:checkpoint has no Lion slots for {len(absent)} of "
              f"{len(store.train_slots)} variables (e.g. {absent[0] + LION_SUFFIX}): the momentum "
              "starts from zero", flush=True)
        m.data.zero_()
        return
    for s in store.train_slots:
        a = np.asarray(tensors[s.name + LION_SUFFIX], dtype=np.float32).reshape(-1)
        if a.size != s.numel:
            raise ValueError(f"{s.name + LION_SUFFIX}: {a.size} elements, expected {s.numel}")
        m.data[s.offset:s.offset + s.numel].copy_(torch.from_numpy(a))


def check_rmsprop_form(tensors: dict, store, centered: bool) -> bool:
    """Whether {TF name: array} holds the slots of an rmsprop run of this form (False: it has
    no ``<name>/RMSProp`` slots for some variable, so the state starts afresh).  Touches
    nothing, so a restore calls it before anything is loaded.  ValueError: the slots are of the
    other form (plain against centered: ``<name>/RMSProp_1`` is the momentum in one and mg in
    the other), or a slot of this form is missing or of the wrong size."""
    names = [s.name for s in store.train_slots]
    if any(n + RMSPROP_SUFFIXES[0] not in tensors for n in names):
        return False
    ckpt_centered = any(n + RMSPROP_SUFFIXES[2] in tensors for n in names)
    if ckpt_centered != centered:
        kind = ("centered", "plain")
        raise ValueError(
            f"checkpoint holds the slots of a {kind[not ckpt_centered]} rmsprop run and this run "
            f"is {kind[not centered]}: {names[0] + RMSPROP_SUFFIXES[1]} is "
            f"{'mg' if ckpt_centered else 'the momentum'} there and "
            f"{'mg' if centered else 'the momentum'} here; restore it with "
            f"--rmsprop_centered={'true' if ckpt_centered else 'false'}")
    for suffix in rmsprop_suffixes(centered).values():
        for s in store.train_slots:
            k = s.name + suffix
            if k not in tensors:
                raise ValueError(f"checkpoint lacks the rmsprop slot {k}")
            size = int(np.asarray(tensors[k]).size)
            if size != s.numel:
                raise ValueError(f"{k}: {size} elements, expected {s.numel}")
    return True


def tf_to_rmsprop(tensors: dict, store, ms: torch.Tensor, mg: torch.Tensor | None,
                  mom: torch.Tensor) -> None:
    """Load the state of an rmsprop run (mg not None: centered) from {TF name: array}.  With
    every slot of its form present they are loaded.  Without the ``<name>/RMSProp`` slots (e.g.
    a `mom` checkpoint, whose ``/Momentum`` is ignored) ms starts from ones, as TF's `rms` slot
    does, mg and mom from zeros, and one log line says so.  A checkpoint of the other form
    (plain into centered or the reverse) is refused: its ``<name>/RMSProp_1`` is the momentum
    in one and mg in the other (check_rmsprop_form, which a restore also calls on its own
    before it loads anything)."""
    centered = mg is not None
    suf = rmsprop_suffixes(centered)
    names = [s.name for s in store.train_slots]
    absent = [n for n in names if n + RMSPROP_SUFFIXES[0] not in tensors]
    if not check_rmsprop_form(tensors, store, centered):
        print(f"INFO:tensorflow:checkpoint has no RMSProp slots for {len(absent)} of "
              f"{len(names)} variables (e.g. {absent[0] + RMSPROP_SUFFIXES[0]}): ms starts from "
              "ones, mg and the momentum from zero", flush=True)
        ms.data.fill_(1.0)
        mom.data.zero_()
        if centered:
            mg.data.zero_()
        return
    for key, buf in (("ms", ms), ("mg", mg), ("mom", mom)):
        if key not in suf:
            continue
        for s in store.train_slots:
            a = np.asarray(tensors[s.name + suf[key]], dtype=np.float32).reshape(-1)
            buf.data[s.offset:s.offset + s.numel].copy_(torch.from_numpy(a))


def ema_weights(tensors: dict, store) -> dict:
    """The tensor dict with every trainable replaced by its EMA shadow (what an
    ``ema.variables_to_restore()`` restore gives TF); BN moving statistics, global_step and
    everything else stay.  KeyError naming the first few when a shadow is missing: a
    checkpoint of a run without --ema_decay is never scored as if it had them."""
    missing = [s.name for s in store.train_slots if s.name + EMA_SUFFIX not in tensors]
    if missing:
        raise KeyError(f"checkpoint lacks the EMA shadows of {len(missing)} variables, e.g. "
                       f"{[m + EMA_SUFFIX for m in missing[:3]]}")
    out = dict(tensors)
    for s in store.train_slots:
        out[s.name] = tensors[s.name + EMA_SUFFIX]
    return out


def tf_to_state(tensors: dict, store, momentum: torch.Tensor | None = None,
                strict: bool = True, ema: torch.Tensor | None = None) -> int:
    """Load {TF name: array} into the ParamStore (+momentum, +EMA shadows); returns
    global_step.  ``ema``: the flat shadow buffer of a run with --ema_decay > 0; a checkpoint
    without (all of) the ``<name>/ExponentialMovingAverage`` entries starts every shadow
    from the restored weights, with one log line.  Without ``ema`` the entries are ignored."""
    missing = []
    for s in store.train_slots + store.stat_slots:
        if s.name not in tensors:
            missing.append(s.name)
            continue
        a = np.asarray(tensors[s.name], dtype=np.float32).reshape(s.shape)
        buf = store.master if s in store.train_slots else store.stats
        buf.data[s.offset:s.offset + s.numel].copy_(torch.from_numpy(a.reshape(-1)))
    if momentum is not None:
        for s in store.train_slots:
            k = f"{s.name}/Momentum"
            if k in tensors:
                a = np.asarray(tensors[k], dtype=np.float32).reshape(-1)
                momentum.data[s.offset:s.offset + s.numel].copy_(torch.from_numpy(a))
    if strict and missing:
        raise KeyError(f"checkpoint lacks {len(missing)} variables, e.g. {missing[:3]}")
    if ema is not None:
        absent = [s.name for s in store.train_slots if s.name + EMA_SUFFIX not in tensors]
        if absent:
            print(f"INFO:tensorflow:checkpoint has no EMA shadows for {len(absent)} of "
                  f"{len(store.train_slots)} variables (e.g. {absent[0] + EMA_SUFFIX}): every "
                  "shadow starts from the restored weights", flush=True)
            ema.data.copy_(store.master.detach())
        else:
            for s in store.train_slots:
                a = np.asarray(tensors[s.name + EMA_SUFFIX], dtype=np.float32).reshape(-1)
                if a.size != s.numel:
                    raise ValueError(f"{s.name + EMA_SUFFIX}: {a.size} elements, expected "
                                     f"{s.numel}")
                ema.data[s.offset:s.offset + s.numel].copy_(torch.from_numpy(a))
    gs = int(np.asarray(tensors.get("global_step", 0)))
    store.global_step = gs
    return gs


class Saver:
    def __init__(self, directory: str, max_to_keep: int = 5, basename: str = "model.ckpt"):
        self.dir = directory
        self.max_to_keep = max_to_keep
        self.basename = basename
        os.makedirs(directory, exist_ok=True)
        st = tb.read_checkpoint_state(directory)
        self.kept: list[str] = []
        if st:
            for p in st["all_model_checkpoint_paths"]:
                q = p if os.path.exists(p + ".index") else os.path.join(directory, os.path.basename(p))
                if os.path.exists(q + ".index"):
                    self.kept.append(q)

    def save(self, tensors: dict, global_step: int) -> str:
        prefix = os.path.join(self.dir, f"{self.basename}-{int(global_step)}")
        tb.write_bundle(prefix, tensors)
        if prefix in self.kept:
            self.kept.remove(prefix)
        self.kept.append(prefix)
        while len(self.kept) > self.max_to_keep:
            old = self.kept.pop(0)
            for f in glob.glob(old + ".*"):
                try:
                    os.remove(f)
                except OSError:
                    pass
        tb.write_checkpoint_state(self.dir, prefix, self.kept)
        return prefix

    def latest(self) -> str | None:
        return tb.latest_checkpoint(self.dir)

    @staticmethod
    def restore(prefix: str) -> dict[str, np.ndarray]:
        return tb.read_bundle(prefix)
